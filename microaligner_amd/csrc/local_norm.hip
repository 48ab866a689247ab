// Local contrast normalisation: an image minus its Gaussian-windowed mean over its Gaussian-windowed standard deviation,
// clipped, as float32 or as uint8 around 128, with whole-image counts (include/microaligner_localnorm.h).  Off the measured
// path: nothing in register() or warp() calls it.
//
// The smoothing is the separable window FIR of window_fir.h, twice: over w and w x for the local mean, then over w d d for
// the variance about it.  Four launches over a 16 B/px workspace of four planes:
//   - row pass 1 stages w and w x straight from the image and the weight, one plane after the other through the same LDS
//     tile, into planes 0 and 1 (transposed).  One instantiation per dtype of the image; the weight kind is a wave-uniform
//     branch;
//   - column pass 1 keeps the two filtered planes in registers and ends in mu = Sx / Sw and Sw, planes 2 and 3 (row-major,
//     8 B/px: stage 2 reads them back instead of filtering w a second time, which would cost a plane-pass in each of its
//     two kernels);
//   - row pass 2 stages w d d from the image, the weight, mu and Sw into plane 0 again (row pass 1's planes are dead behind
//     column pass 1 on the stream);
//   - column pass 2 ends in z from the pixel's own x, mu, Sw and w, writes only the outputs that were asked for, and tallies
//     the four counts per wave (call_counts.h).
// Every plane is written over the whole image before the launch that reads it: no byte of the workspace is read as found.
// LDS is sized by r at launch (40 KiB at r = 12, 97 KiB at r = 128).
#include "../../include/microaligner_localnorm.h"
#include "call_counts.h"
#include "weight_map.h"
#include "window_fir.h"

#include <cmath>

namespace {

constexpr int LN_SIDE_MAX = 1 << 24;
constexpr int LN_PLANES = 4;   // of the workspace: two transposed planes of a row pass, then mu and Sw
static_assert(MA_LOCALNORM_MAX_RADIUS == WF_MAX_RADIUS, "the tile of window_fir.h is sized for this radius");

// the image and the weight as the kernels read them
template <typename T>
struct LnIn {
    const T* img;
    const void* weight;
    int kind;
};

// what column pass 2 makes
struct LnOut {
    float* f32;
    unsigned char* u8;
    unsigned long long* counts;   // [4], or NULL
    float floor, clip, scale, min_support;
};

// x and w of a pixel inside the image; -> is it live?
template <typename T>
__device__ __forceinline__ bool ln_pixel(const LnIn<T>& in, size_t i, float& x, float& w)
{
    w = d_weight_px(in.weight, in.kind, i);
    x = (float)in.img[i];
    return w > 0.f && w < INFINITY && d_finite(x);
}

// plane P (0: w, 1: w x) of stage 1 at (x, y), which must lie inside the image
template <int P, typename T>
__device__ __forceinline__ float ln_product1(const LnIn<T>& in, int W, int x, int y)
{
    float v, w;
    if (!ln_pixel(in, (size_t)y * W + x, v, w)) return 0.f;
    return P == 0 ? w : w * v;
}

// w d d of stage 2 at (x, y), which must lie inside the image
template <typename T>
__device__ __forceinline__ float ln_product2(const LnIn<T>& in, const float* __restrict__ mu, const float* __restrict__ sw,
                                             float min_support, int W, int x, int y)
{
    const size_t i = (size_t)y * W + x;
    float v, w;
    if (!ln_pixel(in, i, v, w) || !(sw[i] > min_support)) return 0.f;
    const float d = v - mu[i];
    return (w * d) * d;
}

// Row pass 1.  ws: planes 0 and 1, (W, H) each.
template <typename T>
__global__ __launch_bounds__(64 * WF_NW) void ln_row1_kernel(LnIn<T> in, int H, int W, int r, const float* __restrict__ taps,
                                                             int nbx, float* __restrict__ ws)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = (int)(blockIdx.x % nbx) * WF_S, y0 = (int)(blockIdx.x / nbx) * 64;
    const size_t plane = (size_t)H * W;
    wf_row_plane([=](int, int W, int x, int y) { return ln_product1<0>(in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws);
    wf_row_plane([=](int, int W, int x, int y) { return ln_product1<1>(in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + plane);
}

// Row pass 2.  mu, sw: (H, W); dst: plane 0, (W, H).
template <typename T>
__global__ __launch_bounds__(64 * WF_NW) void ln_row2_kernel(LnIn<T> in, const float* __restrict__ mu,
                                                             const float* __restrict__ sw, float min_support, int H, int W,
                                                             int r, const float* __restrict__ taps, int nbx,
                                                             float* __restrict__ dst)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = (int)(blockIdx.x % nbx) * WF_S, y0 = (int)(blockIdx.x / nbx) * 64;
    wf_row_plane([=](int, int W, int x, int y) { return ln_product2(in, mu, sw, min_support, W, x, y); }, H, W, r, taps, x0, y0,
                 lane, wv, lds, dst);
}

// Column pass 1: mu and Sw.  Block: columns [x0, x0 + 64) x output rows [y0, y0 + WF_S); lane = column, a wave holds WF_R
// rows of 64 columns.  ws: planes 0 and 1, (W, H) each; mu, sw: (H, W).
__global__ __launch_bounds__(64 * WF_NW) void ln_col1_kernel(const float* __restrict__ ws, int H, int W, int r,
                                                             const float* __restrict__ taps, int nbx, float* __restrict__ mu,
                                                             float* __restrict__ sw)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int span = WF_S + 2 * r + 2 * WF_G, pitch = span | 1;
    const int x0 = (int)(blockIdx.x % nbx) * 64, y0 = (int)(blockIdx.x / nbx) * WF_S;
    const size_t plane = (size_t)H * W;
    float S[2][WF_R];
#pragma unroll
    for (int p = 0; p < 2; p++) {
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
#pragma unroll
    for (int q = 0; q < WF_R; q++) {
        const int y = yb + q;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        mu[i] = __fdiv_rn(S[1][q], S[0][q]);
        sw[i] = S[0][q];
    }
}

// Column pass 2 with z, the outputs and the counts.  The same block as column pass 1.  src: plane 0, (W, H).
template <typename T>
__global__ __launch_bounds__(64 * WF_NW) void ln_col2_kernel(const float* __restrict__ src, LnIn<T> in,
                                                             const float* __restrict__ mu, const float* __restrict__ sw,
                                                             int H, int W, int r, const float* __restrict__ taps, int nbx,
                                                             LnOut o)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int span = WF_S + 2 * r + 2 * WF_G, pitch = span | 1;
    const int x0 = (int)(blockIdx.x % nbx) * 64, y0 = (int)(blockIdx.x / nbx) * WF_S;
    float S[WF_R];
    for (int row = wv; row < 64; row += WF_NW) {
        const int x = x0 + row;
        float* line = lds + row * pitch;
        for (int c = lane; c < span; c += 64) {
            const int y = y0 - r - WF_G + c;
            line[c] = (x < W && y >= 0 && y < H) ? src[(size_t)x * H + y] : 0.f;
        }
    }
    __syncthreads();
    d_sym_fir_slide_pk<WF_R, false, false>(lds + lane * pitch, WF_G + r + wv * WF_R, r, taps, S);
    const int x = x0 + lane, yb = y0 + wv * WF_R;
    unsigned n[MA_LOCALNORM_COUNTS] = {0u, 0u, 0u, 0u};   // dropped, unsupported, flat, clipped
#pragma unroll
    for (int q = 0; q < WF_R; q++) {
        const int y = yb + q;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        float v, w;
        const bool live = ln_pixel(in, i, v, w);
        const float s = sw[i];
        const bool supported = live && s > o.min_support;
        float z = NAN;
        if (supported) {
            const float d = v - mu[i];
            const float var = __fdiv_rn(S[q], s);
            z = __fdiv_rn(d, sqrtf(var + o.floor));   // the correctly rounded root, as in texture.hip
            n[2] += var <= o.floor;
            n[3] += fabsf(z) > o.clip;
        }
        const bool has = z == z;
        n[0] += !live;
        n[1] += live && !has;
        if (o.f32) o.f32[i] = !has ? 0.f : (z < -o.clip ? -o.clip : (z > o.clip ? o.clip : z));
        if (o.u8) {
            float t = z * o.scale;
            t = t + 128.f;
            t = fminf(fmaxf(t, 0.f), 255.f);   // a NaN sum (0 * Inf) -> 0: fmaxf takes its other operand
            o.u8[i] = !has ? (unsigned char)128 : (unsigned char)(int)rintf(t);
        }
    }
    if (o.counts) d_wave_tally(o.counts, n);   // wave-uniform; every lane is here
}

template <typename T>
static int ln_launch(ma_ctx* ctx, const void* img, const void* weight, int kind, int H, int W, int r, const WfBuffers& b,
                     const LnOut& o)
{
    WfShape s;
    MA_TRY(wf_shape(H, W, r, "image", reinterpret_cast<const void*>(ln_row1_kernel<T>),
                    reinterpret_cast<const void*>(ln_col1_kernel), &s));
    MA_TRY(wf_shape(H, W, r, "image", reinterpret_cast<const void*>(ln_row2_kernel<T>),
                    reinterpret_cast<const void*>(ln_col2_kernel<T>), &s));
    const LnIn<T> in{(const T*)img, weight, kind};
    const size_t plane = (size_t)H * W;
    float* mu = b.ws + 2 * plane;
    float* sw = b.ws + 3 * plane;
    const dim3 threads(64 * WF_NW);
    hipLaunchKernelGGL(ln_row1_kernel<T>, dim3(s.g_row), threads, s.lds, ctx->stream, in, H, W, r, (const float*)b.aux,
                       s.nbx_row, b.ws);
    hipLaunchKernelGGL(ln_col1_kernel, dim3(s.g_col), threads, s.lds, ctx->stream, (const float*)b.ws, H, W, r,
                       (const float*)b.aux, s.nbx_col, mu, sw);
    hipLaunchKernelGGL(ln_row2_kernel<T>, dim3(s.g_row), threads, s.lds, ctx->stream, in, (const float*)mu, (const float*)sw,
                       o.min_support, H, W, r, (const float*)b.aux, s.nbx_row, b.ws);
    hipLaunchKernelGGL(ln_col2_kernel<T>, dim3(s.g_col), threads, s.lds, ctx->stream, (const float*)b.ws, in, (const float*)mu,
                       (const float*)sw, H, W, r, (const float*)b.aux, s.nbx_col, o);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" int ma_normalize_local(ma_ctx* ctx, const void* img, int dtype, int H, int W, const float* taps_host, int r,
                                  float floor, float clip, const void* weight, int weight_kind, float min_support,
                                  float* out_f32, uint8_t* out_u8, long long* counts_host)
{
    MA_REQUIRE(ctx && img && taps_host, "NULL argument");
    MA_REQUIRE(out_f32 || out_u8, "no output was asked for");
    MA_REQUIRE((const void*)out_f32 != (const void*)out_u8, "out_f32 and out_u8 must be distinct arrays");
    MA_REQUIRE((const void*)out_f32 != img && (const void*)out_u8 != img, "an output must not be the image");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= LN_SIDE_MAX && W <= LN_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_REQUIRE(r >= 1 && r <= MA_LOCALNORM_MAX_RADIUS, "r must be in [1, 128]");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "unknown dtype");
    MA_TRY(ma_weight_check(weight, weight_kind, false, {out_f32, out_u8}, 1, 1));
    MA_REQUIRE(std::isfinite(floor) && floor > 0.f, "floor must be finite and positive");
    MA_REQUIRE(clip > 0.f, "clip must be positive and not NaN");
    MA_REQUIRE(!out_u8 || clip < INFINITY, "an infinite clip has no uint8 output");
    MA_REQUIRE(std::isfinite(min_support) && min_support >= 0.f, "min_support must be finite and not negative");
    // every array is read and written element by element: the rule asks no more than the element's own alignment
    const size_t img_elem = dtype == MA_U8 ? 1 : (dtype == MA_U16 ? 2 : 4);
    const size_t weight_elem = weight_kind == MA_SMOOTH_WEIGHT_F32 ? sizeof(float) : 1;
    MA_REQUIRE_ALIGNED(img, img_elem, "img");
    MA_REQUIRE_ALIGNED(weight, weight_elem, "weight");
    MA_REQUIRE_ALIGNED(out_f32, sizeof(float), "out_f32");
    WfTaps taps;
    MA_TRY(wf_taps(taps_host, r, &taps));
    LnOut o{out_f32, out_u8, nullptr, floor, clip, 127.0f / clip, min_support};
    MA_HIP(hipSetDevice(ctx->device));
    WfBuffers b;
    MA_TRY(wf_acquire(ctx, 0, LN_PLANES, H, W, counts_host ? MA_LOCALNORM_COUNTS : 0, &b));
    o.counts = b.counts;
    hipLaunchKernelGGL(wf_setup_kernel<>, dim3(1), dim3(256), 0, ctx->stream, taps, r, b.aux);
    int rc;
    switch (dtype) {
    case MA_U8: rc = ln_launch<unsigned char>(ctx, img, weight, weight_kind, H, W, r, b, o); break;
    case MA_U16: rc = ln_launch<unsigned short>(ctx, img, weight, weight_kind, H, W, r, b, o); break;
    default: rc = ln_launch<float>(ctx, img, weight, weight_kind, H, W, r, b, o); break;
    }
    return wf_finish(ctx, b, rc, counts_host);
}
