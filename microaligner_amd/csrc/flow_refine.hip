// One regularised Lucas-Kanade step of a flow against the images (include/microaligner_flowrefine.h).  Off the measured
// path: nothing in register() or warp() calls it.
//
// The smoothing is the separable FIR of the flow smoothing and the texture maps (flow_smooth.hip, texture.hip) over the five
// planes w gx gx, w gx gy, w gy gy, w gx e, w gy e with up to 257 taps, in two launches through a 20 B/px workspace that
// holds the row pass's planes TRANSPOSED ((W, H) each), and with the same tile: 64 lines (lanes) x FR_S = FR_NW * FR_R
// outputs along the filtered axis, coalesced staging into LDS [64 lines][pitch], pitch odd, and d_sym_fir_slide_pk per thread
// in the accumulation order of the header.
//   - The row pass stages the products straight from the warped image, the reference and the weight, one plane after the
//     other through the same LDS tile: every staged element reads Wp at itself and its four neighbours, each read clamped
//     into the image, R and the weight (the caches serve the re-reads of the later planes).  One instantiation per dtype of
//     the reference; the weight kind is a wave-uniform branch.
//   - The column pass keeps the five filtered planes in registers and ends in the solve, the clamp and the add: it reads and
//     writes only the 8 B/px flow, and counts invalid and clamped pixels and the largest step with wave reductions, one
//     integer atomic per wave and statistic.
// LDS is sized by r at launch (40 KiB at r = 12, 97 KiB at r = 128).
#include "../../include/microaligner_flowrefine.h"
#include "ma_internal.h"

#include <cmath>

namespace {

constexpr int FR_SIDE_MAX = 1 << 24;
constexpr int FR_NW = 8, FR_R = 16, FR_S = FR_NW * FR_R;   // waves per block, outputs per thread, outputs per line and block
constexpr int FR_G = 2;                                     // guard elements either side of the halo (d_sym_fir_slide_pk)
constexpr int FR_TAPS = 8 + MA_REFINE_MAX_RADIUS + 8;       // floats of a tap table in the MA_TAP layout
constexpr int FR_PLANES = 5;

static inline int fr_span(int r) { return FR_S + 2 * r + 2 * FR_G; }
static inline int fr_pitch(int r) { return fr_span(r) | 1; }

struct FrTaps { float t[MA_REFINE_MAX_RADIUS + 1]; };

__device__ __forceinline__ bool fr_finite(float v) { return fabsf(v) < INFINITY; }

// aux[0 .. FR_TAPS): the taps in the MA_TAP layout
__global__ __launch_bounds__(256) void fr_setup_kernel(FrTaps taps, int r, float* __restrict__ aux)
{
    const int i = threadIdx.x;
    if (i < FR_TAPS) {
        float v = 0.f;
        if (i == 0) v = taps.t[0];
        else if (i >= 8 && i - 7 <= r) v = taps.t[i - 7];
        aux[i] = v;
    }
}

// plane P of the header at (x, y), which must lie inside the image: every read is clamped into it
template <int P, typename T>
__device__ __forceinline__ float fr_product(const T* __restrict__ ref, const float* __restrict__ wp, const void* __restrict__ weight,
                                            int kind, int H, int W, int x, int y)
{
    const size_t row = (size_t)y * W, i = row + x;
    float w = 1.f;
    if (kind == MA_SMOOTH_WEIGHT_F32) w = ((const float*)weight)[i];                          // wave-uniform branches
    else if (kind == MA_SMOOTH_WEIGHT_U8) w = ((const unsigned char*)weight)[i] ? 1.f : 0.f;
    const float c = wp[i], rv = (float)ref[i];
    const float gx = 0.5f * (wp[row + min(x + 1, W - 1)] - wp[row + max(x - 1, 0)]);
    const float gy = 0.5f * (wp[(size_t)min(y + 1, H - 1) * W + x] - wp[(size_t)max(y - 1, 0) * W + x]);
    if (!(w > 0.f && w < INFINITY && fr_finite(c) && fr_finite(rv) && fr_finite(gx) && fr_finite(gy))) return 0.f;
    const float a = w * gx, b = w * gy;
    if (P == 0) return a * gx;
    if (P == 1) return a * gy;
    if (P == 2) return b * gy;
    const float e = c - rv;
    return P == 3 ? a * e : b * e;
}

// one plane of the row pass through the block's LDS tile
template <int P, typename T>
__device__ __forceinline__ void fr_row_plane(const T* __restrict__ ref, const float* __restrict__ wp, const void* __restrict__ weight,
                                             int kind, int H, int W, int r, const float* __restrict__ taps, int x0, int y0,
                                             int lane, int wv, float* lds, float* __restrict__ dst)
{
    const int span = FR_S + 2 * r + 2 * FR_G, pitch = span | 1;
    for (int row = wv; row < 64; row += FR_NW) {
        const int y = y0 + row;
        float* line = lds + row * pitch;
        for (int c = lane; c < span; c += 64) {
            const int x = x0 - r - FR_G + c;
            line[c] = (y < H && x >= 0 && x < W) ? fr_product<P>(ref, wp, weight, kind, H, W, x, y) : 0.f;
        }
    }
    __syncthreads();
    float acc[FR_R];
    d_sym_fir_slide_pk<FR_R, false, false>(lds + lane * pitch, FR_G + r + wv * FR_R, r, taps, acc);
    __syncthreads();
    const int y = y0 + lane;
#pragma unroll
    for (int q = 0; q < FR_R; q++) {
        const int x = x0 + wv * FR_R + q;
        if (x < W && y < H) dst[(size_t)x * H + y] = acc[q];
    }
}

// Row pass.  Block: rows [y0, y0 + 64) x output columns [x0, x0 + FR_S); lane = row.  ws: the five (W, H) planes.
template <typename T>
__global__ __launch_bounds__(64 * FR_NW) void fr_row_kernel(const T* __restrict__ ref, const float* __restrict__ wp,
                                                            const void* __restrict__ weight, int kind, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, float* __restrict__ ws)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = (int)(blockIdx.x % nbx) * FR_S, y0 = (int)(blockIdx.x / nbx) * 64;
    const size_t plane = (size_t)H * W;
    fr_row_plane<0>(ref, wp, weight, kind, H, W, r, taps, x0, y0, lane, wv, lds, ws);
    fr_row_plane<1>(ref, wp, weight, kind, H, W, r, taps, x0, y0, lane, wv, lds, ws + plane);
    fr_row_plane<2>(ref, wp, weight, kind, H, W, r, taps, x0, y0, lane, wv, lds, ws + 2 * plane);
    fr_row_plane<3>(ref, wp, weight, kind, H, W, r, taps, x0, y0, lane, wv, lds, ws + 3 * plane);
    fr_row_plane<4>(ref, wp, weight, kind, H, W, r, taps, x0, y0, lane, wv, lds, ws + 4 * plane);
}

// Column pass with the solve, the clamp and the add.  Block: columns [x0, x0 + 64) x output rows [y0, y0 + FR_S); lane =
// column, a wave holds FR_R rows of 64 columns.  flow and out may be one array: neither is __restrict__, and a thread reads
// flow only at the pixel it writes.  stats: NULL, or { invalid, clamped, bits of step_max }.
__global__ __launch_bounds__(64 * FR_NW) void fr_col_kernel(const float* __restrict__ ws, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, float floor, float max_step,
                                                            const float2* flow, float2* out,
                                                            unsigned long long* __restrict__ stats)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int span = FR_S + 2 * r + 2 * FR_G, pitch = span | 1;
    const int x0 = (int)(blockIdx.x % nbx) * 64, y0 = (int)(blockIdx.x / nbx) * FR_S;
    const size_t plane = (size_t)H * W;
    float S[FR_PLANES][FR_R];
#pragma unroll
    for (int p = 0; p < FR_PLANES; p++) {
        const float* src = ws + p * plane;
        for (int row = wv; row < 64; row += FR_NW) {
            const int x = x0 + row;
            float* line = lds + row * pitch;
            for (int c = lane; c < span; c += 64) {
                const int y = y0 - r - FR_G + c;
                line[c] = (x < W && y >= 0 && y < H) ? src[(size_t)x * H + y] : 0.f;
            }
        }
        __syncthreads();
        d_sym_fir_slide_pk<FR_R, false, false>(lds + lane * pitch, FR_G + r + wv * FR_R, r, taps, S[p]);
        __syncthreads();
    }
    const int x = x0 + lane, yb = y0 + wv * FR_R;
    unsigned invalid = 0, clamped = 0, top = 0;   // top: bits of the largest |component|, which orders as the floats do
#pragma unroll
    for (int q = 0; q < FR_R; q++) {
        const int y = yb + q;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        const float sxy = S[1][q], sxe = S[3][q], sye = S[4][q];
        const float a = S[0][q] + floor, c = S[2][q] + floor;
        const float det = a * c - sxy * sxy;
        float dx = __fdiv_rn(c * sxe - sxy * sye, det), dy = __fdiv_rn(a * sye - sxy * sxe, det);
        if (!(det > 0.f && det < INFINITY && fr_finite(dx) && fr_finite(dy))) {
            dx = dy = 0.f;
            invalid++;
        }
        const float cx = dx > max_step ? max_step : (dx < -max_step ? -max_step : dx);
        const float cy = dy > max_step ? max_step : (dy < -max_step ? -max_step : dy);
        clamped += (cx != dx || cy != dy) ? 1u : 0u;
        top = max(top, max(__float_as_uint(fabsf(cx)), __float_as_uint(fabsf(cy))));
        const float2 f = flow[i];
        out[i] = make_float2(f.x + cx, f.y + cy);
    }
    if (stats) {     // wave-uniform; integer adds and an integer maximum, so the totals do not depend on the order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            invalid += __shfl_down(invalid, off, 64);
            clamped += __shfl_down(clamped, off, 64);
            top = max(top, (unsigned)__shfl_down(top, off, 64));
        }
        if (lane == 0) {
            if (invalid) atomicAdd(stats, (unsigned long long)invalid);
            if (clamped) atomicAdd(stats + 1, (unsigned long long)clamped);
            if (top) atomicMax(stats + 2, (unsigned long long)top);
        }
    }
}

// blocks of a 1-D grid over nbx x nby tiles
static int fr_grid(long long nbx, long long nby, unsigned* blocks)
{
    MA_REQUIRE(nbx * nby <= 0x7fffffffLL, "image too large");
    *blocks = (unsigned)(nbx * nby);
    return MA_OK;
}

template <typename T>
static int fr_launch(ma_ctx* ctx, const void* ref, const float* wp, const void* weight, int kind, int H, int W, int r,
                     const float* aux, float* ws, float floor, float max_step, const float* flow, float* out,
                     unsigned long long* stats)
{
    const size_t lds = (size_t)64 * fr_pitch(r) * sizeof(float);
    const int nbx1 = (W + FR_S - 1) / FR_S, nbx2 = (W + 63) / 64;
    unsigned g1, g2;
    MA_TRY(fr_grid(nbx1, (H + 63) / 64, &g1));
    MA_TRY(fr_grid(nbx2, (H + FR_S - 1) / FR_S, &g2));
    if (lds > 64 * 1024) {
        MA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fr_row_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
        MA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fr_col_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    }
    hipLaunchKernelGGL(fr_row_kernel<T>, dim3(g1), dim3(64 * FR_NW), lds, ctx->stream, (const T*)ref, wp, weight, kind, H, W, r,
                       aux, nbx1, ws);
    hipLaunchKernelGGL(fr_col_kernel, dim3(g2), dim3(64 * FR_NW), lds, ctx->stream, (const float*)ws, H, W, r, aux, nbx2, floor,
                       max_step, (const float2*)flow, (float2*)out, stats);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" int ma_flow_refine_step(ma_ctx* ctx, const void* ref, int dtype, const float* warped, int H, int W,
                                   const float* taps_host, int r, float floor, const void* weight, int weight_kind,
                                   float max_step, const float* flow, float* out, long long* stats_host)
{
    MA_REQUIRE(ctx && ref && warped && taps_host && flow && out, "NULL argument");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FR_SIDE_MAX && W <= FR_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_REQUIRE(r >= 1 && r <= MA_REFINE_MAX_RADIUS, "r must be in [1, 128]");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "unknown dtype");
    MA_REQUIRE(weight_kind == MA_SMOOTH_WEIGHT_NONE || weight_kind == MA_SMOOTH_WEIGHT_F32 || weight_kind == MA_SMOOTH_WEIGHT_U8,
               "the weight must be none or per pixel, float32 or uint8");
    MA_REQUIRE(weight_kind == MA_SMOOTH_WEIGHT_NONE || weight, "NULL weight");
    MA_REQUIRE(ref != (const void*)out && (const void*)warped != (const void*)out, "ref, warped and out must be distinct arrays");
    MA_REQUIRE(weight_kind == MA_SMOOTH_WEIGHT_NONE || weight != (const void*)out, "weight and out must be distinct arrays");
    MA_REQUIRE(std::isfinite(floor) && floor > 0.f, "floor must be finite and positive");
    MA_REQUIRE(std::isfinite(max_step) && max_step > 0.f, "max_step must be finite and positive");
    FrTaps taps{};
    for (int k = 0; k <= r; k++) {
        MA_REQUIRE(std::isfinite(taps_host[k]) && taps_host[k] >= 0.f, "taps must be finite and not negative");
        taps.t[k] = taps_host[k];
    }
    MA_REQUIRE(taps.t[0] > 0.f, "the centre tap must be positive");
    MA_HIP(hipSetDevice(ctx->device));
    unsigned long long* stats = nullptr;
    const size_t stats_bytes = MA_REFINE_STATS * sizeof(unsigned long long);
    if (stats_host) {
        MA_TRY(ma_ws_reserve(ctx, stats_bytes));
        MA_TRY(ma_pinned_reserve(ctx, stats_bytes));
        stats = (unsigned long long*)ctx->ws;
        MA_HIP(hipMemsetAsync(stats, 0, stats_bytes, ctx->stream));
    }
    float* aux = (float*)ma_pool_alloc(ctx, FR_TAPS * sizeof(float));
    if (!aux) return MA_ENOMEM;
    float* ws = (float*)ma_pool_alloc(ctx, (size_t)H * W * FR_PLANES * sizeof(float));
    if (!ws) {
        ma_pool_free(ctx, aux);
        return MA_ENOMEM;
    }
    hipLaunchKernelGGL(fr_setup_kernel, dim3(1), dim3(256), 0, ctx->stream, taps, r, aux);
    int rc;
    switch (dtype) {
    case MA_U8: rc = fr_launch<unsigned char>(ctx, ref, warped, weight, weight_kind, H, W, r, aux, ws, floor, max_step, flow, out, stats); break;
    case MA_U16: rc = fr_launch<unsigned short>(ctx, ref, warped, weight, weight_kind, H, W, r, aux, ws, floor, max_step, flow, out, stats); break;
    default: rc = fr_launch<float>(ctx, ref, warped, weight, weight_kind, H, W, r, aux, ws, floor, max_step, flow, out, stats); break;
    }
    // stream-ordered reuse: the next call on this ctx that takes the buffers runs behind these kernels
    ma_pool_free(ctx, ws);
    ma_pool_free(ctx, aux);
    MA_TRY(rc);
    if (stats_host) {
        MA_HIP(hipMemcpyAsync(ctx->pinned, stats, stats_bytes, hipMemcpyDeviceToHost, ctx->stream));
        MA_HIP(hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < MA_REFINE_STATS; k++) stats_host[k] = (long long)((const unsigned long long*)ctx->pinned)[k];
    }
    return MA_OK;
}
