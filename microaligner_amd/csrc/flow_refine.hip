// One regularised Lucas-Kanade step of a flow against the images (include/microaligner_flowrefine.h).  Off the measured
// path: nothing in register() or warp() calls it.
//
// The smoothing is the separable window FIR of window_fir.h over the five planes w gx gx, w gx gy, w gy gy, w gx e, w gy e
// (a 20 B/px workspace).
//   - The row pass stages the products straight from the warped image, the reference and the weight, one plane after the
//     other through the same LDS tile: every staged element reads Wp at itself and its four neighbours, each read clamped
//     into the image, R and the weight (the caches serve the re-reads of the later planes).  One instantiation per dtype of
//     the reference; the weight kind is a wave-uniform branch.
//   - The column pass keeps the five filtered planes in registers and ends in the solve, the clamp and the add: it reads and
//     writes only the 8 B/px flow, and counts invalid and clamped pixels and the largest step with wave reductions, one
//     integer atomic per wave and statistic: the tally of call_counts.h with a maximum for its third value, so stated here;
//     the host side of the statistics is that header's.
// LDS is sized by r at launch (40 KiB at r = 12, 97 KiB at r = 128).
#include "../../include/microaligner_flowrefine.h"
#include "call_counts.h"
#include "weight_map.h"
#include "window_fir.h"

#include <cmath>

namespace {

constexpr int FR_SIDE_MAX = 1 << 24;
constexpr int FR_PLANES = 5;
static_assert(MA_REFINE_MAX_RADIUS == WF_MAX_RADIUS, "the tile of window_fir.h is sized for this radius");

// plane P of the header at (x, y), which must lie inside the image: every read is clamped into it
template <int P, typename T>
__device__ __forceinline__ float fr_product(const T* __restrict__ ref, const float* __restrict__ wp, const void* __restrict__ weight,
                                            int kind, int H, int W, int x, int y)
{
    const size_t row = (size_t)y * W, i = row + x;
    const float w = d_weight_px(weight, kind, i);
    const float c = wp[i], rv = (float)ref[i];
    const float gx = 0.5f * (wp[row + min(x + 1, W - 1)] - wp[row + max(x - 1, 0)]);
    const float gy = 0.5f * (wp[(size_t)min(y + 1, H - 1) * W + x] - wp[(size_t)max(y - 1, 0) * W + x]);
    if (!(d_weight_counts(w) && d_finite(c) && d_finite(rv) && d_finite(gx) && d_finite(gy))) return 0.f;
    const float a = w * gx, b = w * gy;
    if (P == 0) return a * gx;
    if (P == 1) return a * gy;
    if (P == 2) return b * gy;
    const float e = c - rv;
    return P == 3 ? a * e : b * e;
}

// Row pass.  ws: the five (W, H) planes.
template <typename T>
__global__ __launch_bounds__(64 * WF_NW) void fr_row_kernel(const T* __restrict__ ref, const float* __restrict__ wp,
                                                            const void* __restrict__ weight, int kind, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, float* __restrict__ ws)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = (int)(blockIdx.x % nbx) * WF_S, y0 = (int)(blockIdx.x / nbx) * 64;
    const size_t plane = (size_t)H * W;
    wf_row_plane([=](int H, int W, int x, int y) { return fr_product<0>(ref, wp, weight, kind, H, W, x, y); }, H, W, r, taps, x0,
                 y0, lane, wv, lds, ws);
    wf_row_plane([=](int H, int W, int x, int y) { return fr_product<1>(ref, wp, weight, kind, H, W, x, y); }, H, W, r, taps, x0,
                 y0, lane, wv, lds, ws + plane);
    wf_row_plane([=](int H, int W, int x, int y) { return fr_product<2>(ref, wp, weight, kind, H, W, x, y); }, H, W, r, taps, x0,
                 y0, lane, wv, lds, ws + 2 * plane);
    wf_row_plane([=](int H, int W, int x, int y) { return fr_product<3>(ref, wp, weight, kind, H, W, x, y); }, H, W, r, taps, x0,
                 y0, lane, wv, lds, ws + 3 * plane);
    wf_row_plane([=](int H, int W, int x, int y) { return fr_product<4>(ref, wp, weight, kind, H, W, x, y); }, H, W, r, taps, x0,
                 y0, lane, wv, lds, ws + 4 * plane);
}

// Column pass with the solve, the clamp and the add.  Block: columns [x0, x0 + 64) x output rows [y0, y0 + WF_S); lane =
// column, a wave holds WF_R rows of 64 columns.  flow and out may be one array: neither is __restrict__, and a thread reads
// flow only at the pixel it writes.  stats: NULL, or { invalid, clamped, bits of step_max }.
__global__ __launch_bounds__(64 * WF_NW) void fr_col_kernel(const float* __restrict__ ws, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, float floor, float max_step,
                                                            const float2* flow, float2* out,
                                                            unsigned long long* __restrict__ stats)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int span = WF_S + 2 * r + 2 * WF_G, pitch = span | 1;
    const int x0 = (int)(blockIdx.x % nbx) * 64, y0 = (int)(blockIdx.x / nbx) * WF_S;
    const size_t plane = (size_t)H * W;
    float S[FR_PLANES][WF_R];
#pragma unroll
    for (int p = 0; p < FR_PLANES; p++) {
        const float* src = ws + p * plane;
        for (int row = wv; row < 64; row += WF_NW) {
            const int x = x0 + row;
            float* line = lds + row * pitch;
            for (int c = lane; c < span; c += 64) {
                const int y = y0 - r - WF_G + c;
                line[c] = (x < W && y >= 0 && y < H) ? src[(size_t)x * H + y] : 0.f;
            }
        }
        __syncthreads();
        d_sym_fir_slide_pk<WF_R, false, false>(lds + lane * pitch, WF_G + r + wv * WF_R, r, taps, S[p]);
        __syncthreads();
    }
    const int x = x0 + lane, yb = y0 + wv * WF_R;
    unsigned invalid = 0, clamped = 0, top = 0;   // top: bits of the largest |component|, which orders as the floats do
#pragma unroll
    for (int q = 0; q < WF_R; q++) {
        const int y = yb + q;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        const float sxy = S[1][q], sxe = S[3][q], sye = S[4][q];
        const float a = S[0][q] + floor, c = S[2][q] + floor;
        const float det = a * c - sxy * sxy;
        float dx = __fdiv_rn(c * sxe - sxy * sye, det), dy = __fdiv_rn(a * sye - sxy * sxe, det);
        if (!(det > 0.f && det < INFINITY && d_finite(dx) && d_finite(dy))) {
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

template <typename T>
static int fr_launch(ma_ctx* ctx, const void* ref, const float* wp, const void* weight, int kind, int H, int W, int r,
                     const float* aux, float* ws, float floor, float max_step, const float* flow, float* out,
                     unsigned long long* stats)
{
    WfShape s;
    MA_TRY(wf_shape(H, W, r, "image", reinterpret_cast<const void*>(fr_row_kernel<T>),
                    reinterpret_cast<const void*>(fr_col_kernel), &s));
    hipLaunchKernelGGL(fr_row_kernel<T>, dim3(s.g_row), dim3(64 * WF_NW), s.lds, ctx->stream, (const T*)ref, wp, weight, kind, H,
                       W, r, aux, s.nbx_row, ws);
    hipLaunchKernelGGL(fr_col_kernel, dim3(s.g_col), dim3(64 * WF_NW), s.lds, ctx->stream, (const float*)ws, H, W, r, aux,
                       s.nbx_col, floor, max_step, (const float2*)flow, (float2*)out, stats);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" int ma_flow_refine_step(ma_ctx* ctx, const void* ref, int dtype, const float* warped, int H, int W,
                                   const float* taps_host, int r, float floor, const void* weight, int weight_kind,
                                   float max_step, const float* flow, float* out, long long* stats_host)
{
    MA_REQUIRE(ctx && ref && warped && taps_host && flow && out, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FR_SIDE_MAX && W <= FR_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_REQUIRE(r >= 1 && r <= MA_REFINE_MAX_RADIUS, "r must be in [1, 128]");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "unknown dtype");
    MA_TRY(ma_weight_check(weight, weight_kind, false, {out}, 1, 1));
    MA_REQUIRE(ref != (const void*)out && (const void*)warped != (const void*)out, "ref, warped and out must be distinct arrays");
    MA_REQUIRE(std::isfinite(floor) && floor > 0.f, "floor must be finite and positive");
    MA_REQUIRE(std::isfinite(max_step) && max_step > 0.f, "max_step must be finite and positive");
    WfTaps taps;
    MA_TRY(wf_taps(taps_host, r, &taps));
    MA_HIP(hipSetDevice(ctx->device));
    unsigned long long* stats;
    MA_TRY(ma_call_counts(ctx, stats_host != nullptr, MA_REFINE_STATS, &stats));
    WfBuffers b;
    MA_TRY(wf_acquire(ctx, 0, FR_PLANES, H, W, 0, &b));
    hipLaunchKernelGGL(wf_setup_kernel<>, dim3(1), dim3(256), 0, ctx->stream, taps, r, b.aux);
    int rc;
    switch (dtype) {
    case MA_U8: rc = fr_launch<unsigned char>(ctx, ref, warped, weight, weight_kind, H, W, r, b.aux, b.ws, floor, max_step, flow, out, stats); break;
    case MA_U16: rc = fr_launch<unsigned short>(ctx, ref, warped, weight, weight_kind, H, W, r, b.aux, b.ws, floor, max_step, flow, out, stats); break;
    default: rc = fr_launch<float>(ctx, ref, warped, weight, weight_kind, H, W, r, b.aux, b.ws, floor, max_step, flow, out, stats); break;
    }
    MA_TRY(wf_finish(ctx, b, rc, nullptr));
    if (stats_host) MA_TRY(ma_read_call_counts(ctx, stats, MA_REFINE_STATS, stats_host));
    return MA_OK;
}
