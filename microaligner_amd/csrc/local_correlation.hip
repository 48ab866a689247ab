// Local correlation maps: the Gaussian-windowed ZNCC of a reference image and another image on its grid, a weight made from
// the score and per-cell class counts (include/microaligner_localcorr.h).  Off the measured path: nothing in register() or
// warp() calls it.
//
// The smoothing is the separable window FIR of window_fir.h over the six planes w, w A, w B, w A A, w B B, w A B (a 24 B/px
// workspace).
//   - The row pass stages the products straight from the reference, the other image and the weight, one plane after the
//     other through the same LDS tile (the caches serve the re-reads of the later planes).  One instantiation per dtype of
//     the reference; the weight kind is a wave-uniform branch.
//   - The column pass keeps the six filtered planes in registers and ends in the score, the weight and the classes: it
//     writes only the planes that were asked for, and counts the classes per cell with wave ballots, one integer atomic per
//     wave, cell and class.
// LDS is sized by r at launch (40 KiB at r = 12, 97 KiB at r = 128).
#include "../../include/microaligner_localcorr.h"
#include "cell_grid.h"
#include "weight_map.h"
#include "window_fir.h"

#include <cmath>

namespace {

constexpr int LC_SIDE_MAX = 1 << 24;
constexpr int LC_PLANES = 6;
static_assert(MA_LOCALCORR_MAX_RADIUS == WF_MAX_RADIUS, "the tile of window_fir.h is sized for this radius");

// the scalars of the row pass
struct LcIn {
    const float* img;
    const void* weight;
    int kind;
    float center_ref, center_img;
};

// what the column pass makes; the grid is read for counts
struct LcOut {
    float* score;
    float* weight;
    unsigned long long* counts;   // [gy][gx][4]
    float floor, min_support, lo, hi, span;
    int ch, cw, gx;
};

// plane P of the header at (x, y), which must lie inside the image
template <int P, typename T>
__device__ __forceinline__ float lc_product(const T* __restrict__ ref, const LcIn& in, int W, int x, int y)
{
    const size_t i = (size_t)y * W + x;
    const float w = d_weight_px(in.weight, in.kind, i);
    const float a = (float)ref[i] - in.center_ref, b = in.img[i] - in.center_img;
    if (!(w > 0.f && w < INFINITY && d_finite(a) && d_finite(b))) return 0.f;   // d_weight_counts() compiles to other code here
    if (P == 0) return w;
    const float wa = w * a, wb = w * b;
    if (P == 1) return wa;
    if (P == 2) return wb;
    if (P == 3) return wa * a;
    return P == 4 ? wb * b : wa * b;
}

// Row pass.  ws: the six (W, H) planes.
template <typename T>
__global__ __launch_bounds__(64 * WF_NW) void lc_row_kernel(const T* __restrict__ ref, LcIn in, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, float* __restrict__ ws)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = (int)(blockIdx.x % nbx) * WF_S, y0 = (int)(blockIdx.x / nbx) * 64;
    const size_t plane = (size_t)H * W;
    wf_row_plane([=](int, int W, int x, int y) { return lc_product<0>(ref, in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws);
    wf_row_plane([=](int, int W, int x, int y) { return lc_product<1>(ref, in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + plane);
    wf_row_plane([=](int, int W, int x, int y) { return lc_product<2>(ref, in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + 2 * plane);
    wf_row_plane([=](int, int W, int x, int y) { return lc_product<3>(ref, in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + 3 * plane);
    wf_row_plane([=](int, int W, int x, int y) { return lc_product<4>(ref, in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + 4 * plane);
    wf_row_plane([=](int, int W, int x, int y) { return lc_product<5>(ref, in, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + 5 * plane);
}

// Column pass with the score, the weight and the class counts.  Block: columns [x0, x0 + 64) x output rows
// [y0, y0 + WF_S); lane = column, a wave holds WF_R rows of 64 columns.
__global__ __launch_bounds__(64 * WF_NW) void lc_col_kernel(const float* __restrict__ ws, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, LcOut o)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int span = WF_S + 2 * r + 2 * WF_G, pitch = span | 1;
    const int x0 = (int)(blockIdx.x % nbx) * 64, y0 = (int)(blockIdx.x / nbx) * WF_S;
    const size_t plane = (size_t)H * W;
    float S[LC_PLANES][WF_R];
#pragma unroll
    for (int p = 0; p < LC_PLANES; p++) {
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
    // four bits per row of the wave: 0 agree, 1 disagree, 2 flat, 3 unsupported, 4 outside the image
    unsigned long long cls = 0x4444444444444444ull;
#pragma unroll
    for (int q = 0; q < WF_R; q++) {
        const int y = yb + q;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        const float sw = S[0][q];
        float s = NAN, va = NAN, vb = NAN;
        if (sw > o.min_support) {
            const float ma = __fdiv_rn(S[1][q], sw), mb = __fdiv_rn(S[2][q], sw);
            va = __fdiv_rn(S[3][q], sw) - ma * ma;
            vb = __fdiv_rn(S[4][q], sw) - mb * mb;
            va = va < 0.f ? 0.f : va;
            vb = vb < 0.f ? 0.f : vb;
            const float c = __fdiv_rn(S[5][q], sw) - ma * mb;
            const float den = sqrtf(va + o.floor) * sqrtf(vb + o.floor);   // the correctly rounded root, as in texture.hip
            s = __fdiv_rn(c, den);
            s = s > 1.f ? 1.f : (s < -1.f ? -1.f : s);
        }
        const bool nan = s != s;
        if (o.score) o.score[i] = s;
        if (o.weight) o.weight[i] = (nan || s < o.lo) ? 0.f : (s >= o.hi ? 1.f : __fdiv_rn(s - o.lo, o.span));
        const unsigned long long c = nan ? 3u : ((va <= o.floor && vb <= o.floor) ? 2u : (s >= o.hi ? 0u : 1u));
        cls = (cls & ~(15ull << (4 * q))) | (c << (4 * q));
    }
    if (!o.counts) return;        // wave-uniform
    // All 64 lanes are here.  The lanes of a wave hold 64 consecutive columns, i.e. one column of cells, rarely more; its rows
    // one row of cells, rarely two.  Per column of cells: the lanes in it as a mask, per row the ballots of the four classes
    // under that mask, summed over the rows of one cell in scalar registers, then one atomic per class from lane 0.
    const int cx = x < W ? x / o.cw : -1;
    unsigned long long todo = __ballot(x < W);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int seg = __builtin_amdgcn_readfirstlane(__shfl(cx, leader, 64));
        const unsigned long long mine = __ballot(cx == seg);
        int cy = yb / o.ch;
        int ynext = (cy + 1) * o.ch;   // first row of the next row of cells; ch <= H <= 2^24
        unsigned n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        auto flush = [&]() {
            if (lane == 0) {
                unsigned long long* c = o.counts + ((size_t)cy * o.gx + seg) * MA_LOCALCORR_CLASSES;
                if (n0) atomicAdd(c, (unsigned long long)n0);
                if (n1) atomicAdd(c + 1, (unsigned long long)n1);
                if (n2) atomicAdd(c + 2, (unsigned long long)n2);
                if (n3) atomicAdd(c + 3, (unsigned long long)n3);
            }
            n0 = n1 = n2 = n3 = 0;
        };
#pragma unroll
        for (int q = 0; q < WF_R; q++) {
            const int y = yb + q;
            if (y < H) {             // wave-uniform
                if (y == ynext) {
                    flush();
                    cy++;
                    ynext += o.ch;
                }
                const unsigned c = (unsigned)(cls >> (4 * q)) & 15u;
                n0 += (unsigned)__popcll(__ballot(c == 0u) & mine);
                n1 += (unsigned)__popcll(__ballot(c == 1u) & mine);
                n2 += (unsigned)__popcll(__ballot(c == 2u) & mine);
                n3 += (unsigned)__popcll(__ballot(c == 3u) & mine);
            }
        }
        flush();
        todo &= ~mine;
    }
}

template <typename T>
static int lc_launch(ma_ctx* ctx, const void* ref, const LcIn& in, int H, int W, int r, const float* aux, float* ws,
                     const LcOut& o)
{
    WfShape s;
    MA_TRY(wf_shape(H, W, r, "image", reinterpret_cast<const void*>(lc_row_kernel<T>),
                    reinterpret_cast<const void*>(lc_col_kernel), &s));
    hipLaunchKernelGGL(lc_row_kernel<T>, dim3(s.g_row), dim3(64 * WF_NW), s.lds, ctx->stream, (const T*)ref, in, H, W, r, aux,
                       s.nbx_row, ws);
    hipLaunchKernelGGL(lc_col_kernel, dim3(s.g_col), dim3(64 * WF_NW), s.lds, ctx->stream, (const float*)ws, H, W, r, aux,
                       s.nbx_col, o);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" int ma_local_correlation(ma_ctx* ctx, const void* ref, int dtype, const float* img, int H, int W,
                                    const float* taps_host, int r, float center_ref, float center_img, float floor,
                                    const void* weight, int weight_kind, float min_support, float lo, float hi, float* score,
                                    float* weight_out, int cell_h, int cell_w, long long* counts_host)
{
    MA_REQUIRE(ctx && ref && img && taps_host, "NULL argument");
    MA_REQUIRE(score || weight_out || counts_host, "no output was asked for");
    MA_REQUIRE(!score || score != weight_out, "score and weight_out must be distinct arrays");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= LC_SIDE_MAX && W <= LC_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_REQUIRE(r >= 1 && r <= MA_LOCALCORR_MAX_RADIUS, "r must be in [1, 128]");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "unknown dtype");
    MA_TRY(ma_weight_check(weight, weight_kind, false, {}, 1, 1));   // as before, the outputs are not compared with it
    MA_REQUIRE(std::isfinite(center_ref) && std::isfinite(center_img), "the centres must be finite");
    MA_REQUIRE(std::isfinite(floor) && floor > 0.f, "floor must be finite and positive");
    MA_REQUIRE(std::isfinite(min_support) && min_support >= 0.f, "min_support must be finite and not negative");
    MA_REQUIRE(lo >= -1.f && lo < hi && hi <= 1.f, "lo and hi must satisfy -1 <= lo < hi <= 1");
    WfTaps taps;
    MA_TRY(wf_taps(taps_host, r, &taps));
    const LcIn in{img, weight, weight_kind, center_ref, center_img};
    LcOut o{score, weight_out, nullptr, floor, min_support, lo, hi, hi - lo, 1, 1, 1};
    long long ncells = 0;
    if (counts_host) MA_TRY(ma_cell_counts_grid(H, W, cell_h, cell_w, &o, &ncells));
    MA_HIP(hipSetDevice(ctx->device));
    WfBuffers b;
    MA_TRY(wf_acquire(ctx, 0, LC_PLANES, H, W, (size_t)ncells * MA_LOCALCORR_CLASSES, &b));
    o.counts = b.counts;
    hipLaunchKernelGGL(wf_setup_kernel<>, dim3(1), dim3(256), 0, ctx->stream, taps, r, b.aux);
    int rc;
    switch (dtype) {
    case MA_U8: rc = lc_launch<unsigned char>(ctx, ref, in, H, W, r, b.aux, b.ws, o); break;
    case MA_U16: rc = lc_launch<unsigned short>(ctx, ref, in, H, W, r, b.aux, b.ws, o); break;
    default: rc = lc_launch<float>(ctx, ref, in, H, W, r, b.aux, b.ws, o); break;
    }
    return wf_finish(ctx, b, rc, counts_host);
}
