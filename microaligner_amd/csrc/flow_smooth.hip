// Weighted Gaussian smoothing of a flow and the fold mask (include/microaligner_flowsmooth.h).  Off the measured path:
// nothing in register() or warp() calls it.
//
// The smoothing is the separable window FIR of window_fir.h over the three planes w*u, w*v, w (a 12 B/px workspace).
//   - The row pass stages the planes from the flow (float2 loads) and the weight, one plane after the other.
//   - The column pass keeps the three filtered planes in registers and ends in the divide and the blend: it reads flow and
//     weight again only for the blend, and counts the pixels without support (call_counts.h, as the fold mask's kernels do).
// LDS is sized by r at launch (43 KiB at r = 18, 97 KiB at r = 128).
#include "../../include/microaligner_flowsmooth.h"
#include "call_counts.h"
#include "cell_grid.h"
#include "flow_jacobian.h"
#include "weight_map.h"
#include "window_fir.h"

#include <cmath>
#include <vector>

namespace {

constexpr int FS_SIDE_MAX = 1 << 24;
static_assert(MA_SMOOTH_MAX_RADIUS == WF_MAX_RADIUS, "the tile of window_fir.h is sized for this radius");

// the effective weight w(p) of the header
__device__ __forceinline__ float fs_effective(float wgt, float2 f)
{
    return (d_weight_counts(wgt) && d_finite(f.x) && d_finite(f.y)) ? wgt : 0.f;
}

// the header's rule on an axis of n ones at position x: the samples inside the image are 1, the others 0
__device__ __forceinline__ float fs_rule_of_ones(const WfTaps& taps, int r, int x, int n)
{
    float a = taps.t[0] * 1.f;
    for (int k = 1; k <= r; k++) {
        const float lo = x - k >= 0 ? 1.f : 0.f, hi = x + k < n ? 1.f : 0.f;
        a = a + taps.t[k] * (lo + hi);
    }
    return a;
}

// aux[0 .. WF_TAPS): the taps in the MA_TAP layout; with `ones`: aux[WF_TAPS + x] = rs(x), aux[WF_TAPS + W + y] = cs(y)
__global__ __launch_bounds__(256) void fs_setup_kernel(WfTaps taps, int r, int W, int H, int ones, float* __restrict__ aux)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < WF_TAPS) wf_layout_tap(taps, r, (int)i, aux);
    if (!ones) return;
    if (i < W) aux[WF_TAPS + i] = fs_rule_of_ones(taps, r, (int)i, W);
    else if (i < (long long)W + H) aux[WF_TAPS + i] = fs_rule_of_ones(taps, r, (int)(i - W), H);
}

// Row pass.  Block: rows [y0, y0 + 64) x output columns [x0, x0 + WF_S); lane = row.  ws: the three (W, H) planes.
template <int KIND>
__global__ __launch_bounds__(64 * WF_NW) void fs_row_kernel(const float2* __restrict__ flow, int H, int W, MaWeight wt, int r,
                                                            const float* __restrict__ taps, int nbx, float* __restrict__ ws)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int span = WF_S + 2 * r + 2 * WF_G, pitch = span | 1;
    const int x0 = (int)(blockIdx.x % nbx) * WF_S, y0 = (int)(blockIdx.x / nbx) * 64;
    const size_t plane = (size_t)H * W;
    for (int p = 0; p < 3; p++) {
        for (int row = wv; row < 64; row += WF_NW) {
            const int y = y0 + row;
            float* line = lds + row * pitch;
            for (int c = lane; c < span; c += 64) {
                const int x = x0 - r - WF_G + c;
                float val = 0.f;
                if (y < H && x >= 0 && x < W) {
                    const size_t i = (size_t)y * W + x;
                    const float2 f = flow[i];
                    const float w = fs_effective(d_weight_at<KIND>(wt, i, x, y), f);
                    val = p == 2 ? w : (w > 0.f ? w * (p == 0 ? f.x : f.y) : 0.f);
                }
                line[c] = val;
            }
        }
        __syncthreads();
        float acc[WF_R];
        d_sym_fir_slide_pk<WF_R, false, false>(lds + lane * pitch, WF_G + r + wv * WF_R, r, taps, acc);
        __syncthreads();
        const int y = y0 + lane;
        float* dst = ws + p * plane;
#pragma unroll
        for (int q = 0; q < WF_R; q++) {
            const int x = x0 + wv * WF_R + q;
            if (x < W && y < H) dst[(size_t)x * H + y] = acc[q];
        }
    }
}

// Column pass with the divide and the blend.  Block: columns [x0, x0 + 64) x output rows [y0, y0 + WF_S); lane = column.
// flow and out may be one array: neither is __restrict__, and a thread reads flow only at the pixel it writes.
template <int KIND, int MODE>
__global__ __launch_bounds__(64 * WF_NW) void fs_col_kernel(const float* __restrict__ ws, int H, int W, const float2* flow,
                                                            MaWeight wt, int r, const float* __restrict__ aux, int nbx,
                                                            float min_support, float2* out,
                                                            unsigned long long* __restrict__ unsupported)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int span = WF_S + 2 * r + 2 * WF_G, pitch = span | 1;
    const int x0 = (int)(blockIdx.x % nbx) * 64, y0 = (int)(blockIdx.x / nbx) * WF_S;
    const size_t plane = (size_t)H * W;
    float S[3][WF_R];
#pragma unroll
    for (int p = 0; p < 3; p++) {
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
        d_sym_fir_slide_pk<WF_R, false, false>(lds + lane * pitch, WF_G + r + wv * WF_R, r, aux, S[p]);
        __syncthreads();
    }
    const int x = x0 + lane;
    unsigned int missed = 0;
    const float rs = (MODE == MA_SMOOTH_BLEND && x < W) ? aux[WF_TAPS + x] : 1.f;
#pragma unroll
    for (int q = 0; q < WF_R; q++) {
        const int y = y0 + wv * WF_R + q;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        const float s2 = S[2][q];
        float2 s = make_float2(NAN, NAN);
        if (s2 > min_support) s = make_float2(__fdiv_rn(S[0][q], s2), __fdiv_rn(S[1][q], s2));
        else missed++;
        if (MODE == MA_SMOOTH_BLEND) {
            const float2 f = flow[i];
            const float w = fs_effective(d_weight_at<KIND>(wt, i, x, y), f);
            if (w > 0.f) {
                const float sn = aux[WF_TAPS + W + y] * rs;
                const float c = __fdiv_rn(s2, sn);
                const float d = 4.f * c - 2.f;
                const float a = d > 0.f ? (d < 1.f ? d : 1.f) : 0.f;
                if (a == 1.f) s = f;
                else s = make_float2(s.x + a * (f.x - s.x), s.y + a * (f.y - s.y));
            }
        }
        out[i] = s;
    }
    if (unsupported) d_wave_tally(unsupported, {missed});     // wave-uniform
}

// ---- fold mask ------------------------------------------------------------------------------------------------------------
// bad(p) of the header as a byte map, and the folded / invalid counts (counts[0], counts[1]).  One pixel per thread; the
// stencil's four neighbours come from the caches.
__global__ __launch_bounds__(256) void fs_bad_kernel(const float2* __restrict__ flow, int H, int W, int nbx,
                                                     unsigned char* __restrict__ bad, unsigned long long* __restrict__ counts)
{
    const int x = (int)(blockIdx.x % nbx) * 256 + threadIdx.x;
    const int y = (int)(blockIdx.x / nbx);
    unsigned int folded = 0, invalid = 0;
    if (x < W) {
        const size_t i = (size_t)y * W + x;
        const float2 f = flow[i];
        const double det = ma_flow_det_j([&](int dx, int dy) { return flow[(size_t)(y + dy) * W + (x + dx)]; }, x, y, W, H);
        folded = ma_finite(det) && det <= 0.0;
        invalid = !(d_finite(f.x) && d_finite(f.y));
        bad[i] = (folded | invalid) ? 1 : 0;
    }
    d_wave_tally(counts, {folded, invalid});
}

// keep = 1 - (bad dilated by the (2 margin + 1)^2 box), separably through LDS: the bad bytes of the tile and its margin,
// then their OR along x, then along y.  counts[2] = pixels with keep == 0.
constexpr int FM_TW = 64, FM_TH = 32, FM_M = MA_FOLD_MASK_MAX_MARGIN;
__global__ __launch_bounds__(256) void fs_dilate_kernel(const unsigned char* __restrict__ bad, int H, int W, int margin, int nbx,
                                                        unsigned char* __restrict__ keep, unsigned long long* __restrict__ counts)
{
    __shared__ unsigned char sb[FM_TH + 2 * FM_M][FM_TW + 2 * FM_M];
    __shared__ unsigned char sh[FM_TH + 2 * FM_M][FM_TW];
    const int x0 = (int)(blockIdx.x % nbx) * FM_TW, y0 = (int)(blockIdx.x / nbx) * FM_TH;
    const int rows = FM_TH + 2 * margin, cols = FM_TW + 2 * margin;
    for (int t = threadIdx.x; t < rows * cols; t += 256) {
        const int j = t / cols, c = t - j * cols;
        const int y = y0 - margin + j, x = x0 - margin + c;
        sb[j][c] = (y >= 0 && y < H && x >= 0 && x < W) ? bad[(size_t)y * W + x] : 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < rows * FM_TW; t += 256) {
        const int j = t / FM_TW, c = t - j * FM_TW;
        unsigned char any = 0;
        for (int d = 0; d <= 2 * margin; d++) any |= sb[j][c + d];
        sh[j][c] = any;
    }
    __syncthreads();
    unsigned int dropped = 0;
    for (int t = threadIdx.x; t < FM_TH * FM_TW; t += 256) {
        const int j = t / FM_TW, c = t - j * FM_TW;
        const int y = y0 + j, x = x0 + c;
        unsigned char any = 0;
        for (int d = 0; d <= 2 * margin; d++) any |= sh[j + d][c];
        if (y < H && x < W) {
            keep[(size_t)y * W + x] = any ? 0 : 1;
            dropped += any ? 1u : 0u;
        }
    }
    d_wave_tally(counts + 2, {dropped});
}

template <int KIND>
static int fs_launch(ma_ctx* ctx, const float* flow, int H, int W, const MaWeight& wt, int r, int mode, float min_support,
                     const float* aux, float* ws, float* out, unsigned long long* counter)
{
    const void* col = mode == MA_SMOOTH_BLEND ? reinterpret_cast<const void*>(fs_col_kernel<KIND, MA_SMOOTH_BLEND>)
                                              : reinterpret_cast<const void*>(fs_col_kernel<KIND, MA_SMOOTH_ALL>);
    WfShape s;
    MA_TRY(wf_shape(H, W, r, "flow", reinterpret_cast<const void*>(fs_row_kernel<KIND>), col, &s));
    hipLaunchKernelGGL(fs_row_kernel<KIND>, dim3(s.g_row), dim3(64 * WF_NW), s.lds, ctx->stream, (const float2*)flow, H, W, wt, r,
                       aux, s.nbx_row, ws);
    if (mode == MA_SMOOTH_BLEND)
        hipLaunchKernelGGL((fs_col_kernel<KIND, MA_SMOOTH_BLEND>), dim3(s.g_col), dim3(64 * WF_NW), s.lds, ctx->stream,
                           (const float*)ws, H, W, (const float2*)flow, wt, r, aux, s.nbx_col, min_support, (float2*)out, counter);
    else
        hipLaunchKernelGGL((fs_col_kernel<KIND, MA_SMOOTH_ALL>), dim3(s.g_col), dim3(64 * WF_NW), s.lds, ctx->stream,
                           (const float*)ws, H, W, (const float2*)flow, wt, r, aux, s.nbx_col, min_support, (float2*)out, counter);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" int ma_smooth_flow(ma_ctx* ctx, const float* flow, int H, int W, const float* taps_host, int r, const void* weight,
                              int weight_kind, int cell_h, int cell_w, int mode, float min_support, float* out,
                              long long* unsupported_host)
{
    MA_REQUIRE(ctx && flow && taps_host && out, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FS_SIDE_MAX && W <= FS_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(r >= 1 && r <= MA_SMOOTH_MAX_RADIUS, "r must be in [1, 128]");
    MA_TRY(ma_weight_check(weight, weight_kind, true, {out}, cell_h, cell_w));
    MA_REQUIRE(mode == MA_SMOOTH_ALL || mode == MA_SMOOTH_BLEND, "unknown mode");
    MA_REQUIRE(std::isfinite(min_support) && min_support >= 0.f, "min_support must be finite and not negative");
    WfTaps taps;
    MA_TRY(wf_taps(taps_host, r, &taps));
    MA_HIP(hipSetDevice(ctx->device));
    unsigned long long* counter;
    MA_TRY(ma_call_counts(ctx, unsupported_host != nullptr, 1, &counter));
    const int ones = mode == MA_SMOOTH_BLEND ? 1 : 0;
    const size_t tail = ones ? (size_t)W + H : 0;
    WfBuffers b;
    MA_TRY(wf_acquire(ctx, tail, 3, H, W, 0, &b));
    const MaWeight wt = ma_weight_map(weight, weight_kind, W, cell_h, cell_w);
    hipLaunchKernelGGL(fs_setup_kernel, dim3((unsigned)((WF_TAPS + tail + 255) / 256)), dim3(256), 0, ctx->stream, taps, r, W, H,
                       ones, b.aux);
    const int rc = ma_weight_dispatch(weight_kind, [&](auto kind) {
        return fs_launch<kind()>(ctx, flow, H, W, wt, r, mode, min_support, b.aux, b.ws, out, counter);
    });
    MA_TRY(wf_finish(ctx, b, rc, nullptr));
    if (unsupported_host) MA_TRY(ma_read_call_counts(ctx, counter, 1, unsupported_host));
    return MA_OK;
}

extern "C" int ma_flow_fold_mask(ma_ctx* ctx, const float* flow, int H, int W, int margin, unsigned char* keep,
                                 long long* counts_host)
{
    MA_REQUIRE(ctx && flow && keep, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FS_SIDE_MAX && W <= FS_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(margin >= 0 && margin <= MA_FOLD_MASK_MAX_MARGIN, "margin must be in [0, 32]");
    const int nbx1 = (W + 255) / 256, nbx2 = (W + FM_TW - 1) / FM_TW;
    unsigned g1, g2;
    MA_TRY(wf_grid(nbx1, H, "flow", &g1));
    MA_TRY(wf_grid(nbx2, (H + FM_TH - 1) / FM_TH, "flow", &g2));
    MA_HIP(hipSetDevice(ctx->device));
    // the counters are always kept on the device (the kernels add to them); read back only on request
    unsigned long long* counter;
    MA_TRY(ma_call_counts(ctx, true, 3, &counter));
    unsigned char* bad = (unsigned char*)ma_pool_alloc(ctx, (size_t)H * W);
    if (!bad) return MA_ENOMEM;
    hipLaunchKernelGGL(fs_bad_kernel, dim3(g1), dim3(256), 0, ctx->stream, (const float2*)flow, H, W, nbx1, bad, counter);
    hipLaunchKernelGGL(fs_dilate_kernel, dim3(g2), dim3(256), 0, ctx->stream, (const unsigned char*)bad, H, W, margin, nbx2, keep,
                       counter);
    ma_pool_free(ctx, bad);
    MA_HIP(hipGetLastError());
    if (counts_host) MA_TRY(ma_read_call_counts(ctx, counter, 3, counts_host));
    return MA_OK;
}
