// Texture support maps: the eigenvalues of the Gaussian-windowed structure tensor of an image, a weight made from the smaller
// one and per-cell class counts (include/microaligner_texture.h).  Off the measured path: nothing in register() or warp()
// calls it.
//
// The smoothing is the separable window FIR of window_fir.h over the three planes gx*gx, gx*gy, gy*gy (a 12 B/px workspace).
//   - The row pass stages the products straight from the image, one plane after the other through the same LDS tile: every
//     staged element reads I at its two neighbours along x, along y, or both, each read clamped into the image (the caches
//     serve the re-reads; gx and gy are formed again for the plane that needs both).
//   - The column pass keeps the three filtered planes in registers and ends in the eigenvalues: it writes only the planes
//     that were asked for, and counts the classes per cell with wave ballots, one integer atomic per wave, cell and class.
// LDS is sized by r at launch (58 KiB at r = 49, 97 KiB at r = 128).
#include "../../include/microaligner_texture.h"
#include "cell_grid.h"
#include "window_fir.h"

#include <cmath>

namespace {

constexpr int TX_SIDE_MAX = 1 << 24;
static_assert(MA_TEXTURE_MAX_RADIUS == WF_MAX_RADIUS, "the tile of window_fir.h is sized for this radius");

// which outputs the column pass makes; floor is read for weight and counts, the grid for counts
struct TxOut {
    float* lam_min;
    float* lam_max;
    float* weight;
    unsigned long long* counts;   // [gy][gx][3]
    float floor;
    int ch, cw, gx;
};

// plane P of the header at (x, y), which must lie inside the image: every read is clamped into it
template <int P, typename T>
__device__ __forceinline__ float tx_product(const T* __restrict__ img, int H, int W, int x, int y)
{
    const size_t row = (size_t)y * W;
    float gx = 0.f, gy = 0.f;
    if (P <= 1) gx = 0.5f * ((float)img[row + min(x + 1, W - 1)] - (float)img[row + max(x - 1, 0)]);
    if (P >= 1) gy = 0.5f * ((float)img[(size_t)min(y + 1, H - 1) * W + x] - (float)img[(size_t)max(y - 1, 0) * W + x]);
    return P == 0 ? gx * gx : (P == 1 ? gx * gy : gy * gy);
}

// Row pass.  ws: the three (W, H) planes.
template <typename T>
__global__ __launch_bounds__(64 * WF_NW) void tx_row_kernel(const T* __restrict__ img, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, float* __restrict__ ws)
{
    extern __shared__ float lds[];   // [64][pitch]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = (int)(blockIdx.x % nbx) * WF_S, y0 = (int)(blockIdx.x / nbx) * 64;
    const size_t plane = (size_t)H * W;
    wf_row_plane([=](int H, int W, int x, int y) { return tx_product<0>(img, H, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws);
    wf_row_plane([=](int H, int W, int x, int y) { return tx_product<1>(img, H, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + plane);
    wf_row_plane([=](int H, int W, int x, int y) { return tx_product<2>(img, H, W, x, y); }, H, W, r, taps, x0, y0, lane, wv, lds, ws + 2 * plane);
}

// Column pass with the eigenvalues, the weight and the class counts.  Block: columns [x0, x0 + 64) x output rows
// [y0, y0 + WF_S); lane = column, a wave holds WF_R rows of 64 columns.
__global__ __launch_bounds__(64 * WF_NW) void tx_col_kernel(const float* __restrict__ ws, int H, int W, int r,
                                                            const float* __restrict__ taps, int nbx, TxOut o)
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
        d_sym_fir_slide_pk<WF_R, false, false>(lds + lane * pitch, WF_G + r + wv * WF_R, r, taps, S[p]);
        __syncthreads();
    }
    const int x = x0 + lane, yb = y0 + wv * WF_R;
    unsigned cls = 0xffffffffu;   // two bits per row of the wave: 0 textured, 1 edge, 2 flat, 3 outside the image
#pragma unroll
    for (int q = 0; q < WF_R; q++) {
        const int y = yb + q;
        if (x >= W || y >= H) continue;
        const size_t i = (size_t)y * W + x;
        const float sxx = S[0][q], sxy = S[1][q], syy = S[2][q];
        const float h = 0.5f * (sxx + syy), d = 0.5f * (sxx - syy);
        const float rt = sqrtf(d * d + sxy * sxy);   // the correctly rounded root (__fsqrt_rn is the 1 ulp v_sqrt_f32 here)
        const float lmax = h + rt, m = h - rt;
        const float lmin = m < 0.f ? 0.f : m;
        if (o.lam_min) o.lam_min[i] = lmin;
        if (o.lam_max) o.lam_max[i] = lmax;
        if (o.weight) o.weight[i] = lmin > 0.f ? __fdiv_rn(lmin, lmin + o.floor) : 0.f;
        const unsigned c = lmin > o.floor ? 0u : ((lmin <= o.floor && lmax > o.floor) ? 1u : 2u);
        cls = (cls & ~(3u << (2 * q))) | (c << (2 * q));
    }
    if (!o.counts) return;        // wave-uniform
    // All 64 lanes are here.  The lanes of a wave hold 64 consecutive columns, i.e. one column of cells, rarely more; its rows
    // one row of cells, rarely two.  Per column of cells: the lanes in it as a mask, per row the ballots of the three classes
    // under that mask, summed over the rows of one cell in scalar registers, then one atomic per class from lane 0.
    const int cx = x < W ? x / o.cw : -1;
    unsigned long long todo = __ballot(x < W);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int seg = __builtin_amdgcn_readfirstlane(__shfl(cx, leader, 64));
        const unsigned long long mine = __ballot(cx == seg);
        int cy = yb / o.ch;
        int ynext = (cy + 1) * o.ch;   // first row of the next row of cells; ch <= H <= 2^24
        unsigned n0 = 0, n1 = 0, n2 = 0;
        auto flush = [&]() {
            if (lane == 0) {
                unsigned long long* c = o.counts + ((size_t)cy * o.gx + seg) * MA_TEXTURE_CLASSES;
                if (n0) atomicAdd(c, (unsigned long long)n0);
                if (n1) atomicAdd(c + 1, (unsigned long long)n1);
                if (n2) atomicAdd(c + 2, (unsigned long long)n2);
            }
            n0 = n1 = n2 = 0;
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
                const unsigned c = (cls >> (2 * q)) & 3u;
                n0 += (unsigned)__popcll(__ballot(c == 0u) & mine);
                n1 += (unsigned)__popcll(__ballot(c == 1u) & mine);
                n2 += (unsigned)__popcll(__ballot(c == 2u) & mine);
            }
        }
        flush();
        todo &= ~mine;
    }
}

template <typename T>
static int tx_launch(ma_ctx* ctx, const void* img, int H, int W, int r, const float* aux, float* ws, const TxOut& o)
{
    WfShape s;
    MA_TRY(wf_shape(H, W, r, "image", reinterpret_cast<const void*>(tx_row_kernel<T>),
                    reinterpret_cast<const void*>(tx_col_kernel), &s));
    hipLaunchKernelGGL(tx_row_kernel<T>, dim3(s.g_row), dim3(64 * WF_NW), s.lds, ctx->stream, (const T*)img, H, W, r, aux,
                       s.nbx_row, ws);
    hipLaunchKernelGGL(tx_col_kernel, dim3(s.g_col), dim3(64 * WF_NW), s.lds, ctx->stream, (const float*)ws, H, W, r, aux,
                       s.nbx_col, o);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" int ma_texture_maps(ma_ctx* ctx, const void* img, int dtype, int H, int W, const float* taps_host, int r, float floor,
                               float* lam_min, float* lam_max, float* weight, int cell_h, int cell_w, long long* counts_host)
{
    MA_REQUIRE(ctx && img && taps_host, "NULL argument");
    MA_REQUIRE(lam_min || lam_max || weight || counts_host, "no output was asked for");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= TX_SIDE_MAX && W <= TX_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_REQUIRE(r >= 1 && r <= MA_TEXTURE_MAX_RADIUS, "r must be in [1, 128]");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "unknown dtype");
    WfTaps taps;
    MA_TRY(wf_taps(taps_host, r, &taps));
    TxOut o{lam_min, lam_max, weight, nullptr, INFINITY, 1, 1, 1};
    if (weight || counts_host) {
        MA_REQUIRE(std::isfinite(floor) && floor > 0.f, "floor must be finite and positive");
        o.floor = floor;
    }
    long long ncells = 0;
    if (counts_host) MA_TRY(ma_cell_counts_grid(H, W, cell_h, cell_w, &o, &ncells));
    MA_HIP(hipSetDevice(ctx->device));
    WfBuffers b;
    MA_TRY(wf_acquire(ctx, 0, 3, H, W, (size_t)ncells * MA_TEXTURE_CLASSES, &b));
    o.counts = b.counts;
    hipLaunchKernelGGL(wf_setup_kernel<>, dim3(1), dim3(256), 0, ctx->stream, taps, r, b.aux);
    int rc;
    switch (dtype) {
    case MA_U8: rc = tx_launch<unsigned char>(ctx, img, H, W, r, b.aux, b.ws, o); break;
    case MA_U16: rc = tx_launch<unsigned short>(ctx, img, H, W, r, b.aux, b.ws, o); break;
    default: rc = tx_launch<float>(ctx, img, H, W, r, b.aux, b.ws, o); break;
    }
    return wf_finish(ctx, b, rc, counts_host);
}
