// cv2.remap's INTER_NEAREST, INTER_CUBIC and INTER_LANCZOS4 (include/microaligner_interp.h) for the generic remap, the
// tiled warp of Warper.warp() and the page-warp driver.  Off the measured path: remap.hip keeps the linear kernels, and
// MA_INTER_LINEAR forwards to them.
//
// Coordinates are quantised by remap_common.h's quantise() (1/32 px, cvRound); nearest rounds each coordinate on its own.
// The 1-D weight tables are built once per device on the host (interpolateCubic in float, interpolateLanczos4 with sin /
// cos in double) and staged in LDS by every block; u8 forms its 15-bit 2-D weights from them plus the one correction of
// initInterTab2D's sum fix-up, a (tap, delta) pair per fraction pair.  Every sample picks OpenCV's summation order: all
// taps inside the source -> rows left to right, then the row sums; otherwise the taps inside the source one by one.
// Direct gathers, as the linear kernels: several rows per thread, a wave-wide "all taps inside window and image" vote
// selects a straight-line path whose loads are all issued before the first sum.
#include "remap_interp.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace {

// ---- generic cv2.remap --------------------------------------------------------------------------------------------
template <typename T, int MODE, int CN>
__global__ __launch_bounds__(256) void remap_interp_kernel(const T* __restrict__ src, int sh, int sw,
                                                           const float2* __restrict__ map, int dh, int dw,
                                                           T* __restrict__ dst)
{
    constexpr int N = Mode<MODE>::N, OFF = Mode<MODE>::OFF;
    __shared__ float s_tab[TAB * N];
    load_tab<N>(s_tab);
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const float2 m = map[(size_t)y * dw + x];
    T out[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = (T)0;
    if constexpr (MODE == MA_INTER_NEAREST) {
        const int X = d_sat_short(d_cvround(m.x)), Y = d_sat_short(d_cvround(m.y));
        if ((unsigned)X < (unsigned)sw && (unsigned)Y < (unsigned)sh) {
#pragma unroll
            for (int c = 0; c < CN; c++) out[c] = src[((size_t)Y * sw + X) * CN + c];
        }
    } else {
        const Tap t = quantise(m.x, m.y);
        const int sx = t.sx - OFF, sy = t.sy - OFF;
        if (!(sx >= sw || sx + N <= 0 || sy >= sh || sy + N <= 0)) {
            const bool fast = d_below(sx, sw - N + 1) && d_below(sy, sh - N + 1);
            unsigned rmask = 0, cmask = 0;
#pragma unroll
            for (int k = 0; k < N; k++) {
                rmask |= (unsigned)((unsigned)(sy + k) < (unsigned)sh) << k;
                cmask |= (unsigned)((unsigned)(sx + k) < (unsigned)sw) << k;
            }
#pragma unroll
            for (int c = 0; c < CN; c++) {
                T v[N][N];
#pragma unroll
                for (int k1 = 0; k1 < N; k1++)
#pragma unroll
                    for (int k2 = 0; k2 < N; k2++)
                        v[k1][k2] = ((rmask >> k1) & (cmask >> k2) & 1u) ? src[((size_t)(sy + k1) * sw + (sx + k2)) * CN + c]
                                                                          : (T)0;
                out[c] = combine<T, N>(v, s_tab, t.fx, t.fy, fast, rmask, cmask);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CN; c++) dst[((size_t)y * dw + x) * CN + c] = out[c];
}

// ---- Warper.warp(): window-local map = float(x_local) - flow, the zero-padded window is the source ------------------
// (the window origins are remap_common.h's, shared with the linear kernels)

// one sample of the window at (ox, oy), tap origin (sx, sy) window-local: taps beyond the window are not read (skipped
// by the sum unless every tap is inside it), taps in the window's zero padding read 0
template <typename T, int N>
__device__ __forceinline__ T warp_interp_px(const T* __restrict__ img, const MaTiling& g, const Tap& t, int sx, int sy,
                                            int ox, int oy, const float* s_tab)
{
    if (sx >= g.Pw || sx + N <= 0 || sy >= g.Ph || sy + N <= 0) return (T)0;
    const bool fast = d_below(sx, g.Pw - N + 1) && d_below(sy, g.Ph - N + 1);
    unsigned rmask = 0, cmask = 0, rimg = 0, cimg = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
        rmask |= (unsigned)((unsigned)(sy + k) < (unsigned)g.Ph) << k;
        cmask |= (unsigned)((unsigned)(sx + k) < (unsigned)g.Pw) << k;
        rimg |= (unsigned)((unsigned)(oy + sy + k) < (unsigned)g.H) << k;
        cimg |= (unsigned)((unsigned)(ox + sx + k) < (unsigned)g.W) << k;
    }
    const unsigned rok = rmask & rimg, cok = cmask & cimg;
    T v[N][N];
#pragma unroll
    for (int k1 = 0; k1 < N; k1++)
#pragma unroll
        for (int k2 = 0; k2 < N; k2++)
            v[k1][k2] = ((rok >> k1) & (cok >> k2) & 1u) ? img[(size_t)(oy + sy + k1) * g.W + (ox + sx + k2)] : (T)0;
    return combine<T, N>(v, s_tab, t.fx, t.fy, fast, rmask, cmask);
}

// Output rows [y_begin, y_end) of the tiled warp (the whole image for ma_warp_tiled_interp, one band for the page driver).
// R rows per thread; block rows beyond the grid's y extent loop (gridDim.y is capped).
template <typename T, int MODE, bool IDX32>
__global__ __launch_bounds__(256) void warp_interp_kernel(const T* __restrict__ img, MaTiling g,
                                                          const float2* __restrict__ flow, T* __restrict__ out,
                                                          int y_begin, int y_end)
{
    constexpr int N = Mode<MODE>::N, OFF = Mode<MODE>::OFF, R = Mode<MODE>::R;
    __shared__ float s_tab[TAB * N];
    load_tab<N>(s_tab);
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int ox = warp_window_origin_x(min(x, g.W - 1), g);     // (all lanes: the wave's first lane decides)
    if (x >= g.W) return;
    const int lx = x - ox;
    for (int y0 = y_begin + (int)blockIdx.y * R; y0 < y_end; y0 += (int)gridDim.y * R) {
        const WarpRowsY rows(y0, g);
        float2 f[R];
        int ys[R], oys[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            ys[r] = min(y0 + r, y_end - 1);
            oys[r] = rows.origin(ys[r]);
            f[r] = flow[(size_t)ys[r] * g.W + x];
        }
        T res[R];
        if constexpr (MODE == MA_INTER_NEAREST) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                // warper.py:57-59: float32(float64(-flow) + arange) == the correctly rounded lx - flow
                const int X = d_sat_short(d_cvround((float)lx - f[r].x)), Y = d_sat_short(d_cvround((float)(ys[r] - oys[r]) - f[r].y));
                const int jx = ox + X, jy = oys[r] + Y;
                const bool ok = (unsigned)X < (unsigned)g.Pw && (unsigned)Y < (unsigned)g.Ph && (unsigned)jx < (unsigned)g.W &&
                                (unsigned)jy < (unsigned)g.H;
                res[r] = ok ? img[(size_t)jy * g.W + jx] : (T)0;
            }
        } else {
            Tap t[R];
            int sx[R], sy[R];
            bool inside = true;
#pragma unroll
            for (int r = 0; r < R; r++) {
                t[r] = quantise((float)lx - f[r].x, (float)(ys[r] - oys[r]) - f[r].y);
                sx[r] = t[r].sx - OFF; sy[r] = t[r].sy - OFF;
                inside = inside && d_below(sx[r], g.Pw - N + 1) && d_below(sy[r], g.Ph - N + 1) &&
                         d_below(ox + sx[r], g.W - N + 1) && d_below(oys[r] + sy[r], g.H - N + 1);
            }
            if (__all(inside)) {
                // every tap of every row of the wave inside both window and image: OpenCV's straight path, loads first
                T v[R][N][N];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if (IDX32) {
                        const unsigned p = (unsigned)(oys[r] + sy[r]) * (unsigned)g.W + (unsigned)(ox + sx[r]);
#pragma unroll
                        for (int k1 = 0; k1 < N; k1++)
#pragma unroll
                            for (int k2 = 0; k2 < N; k2++) v[r][k1][k2] = img[p + (unsigned)k1 * (unsigned)g.W + (unsigned)k2];
                    } else {
                        const T* q = img + (size_t)(oys[r] + sy[r]) * g.W + (ox + sx[r]);
#pragma unroll
                        for (int k1 = 0; k1 < N; k1++)
#pragma unroll
                            for (int k2 = 0; k2 < N; k2++) v[r][k1][k2] = q[(size_t)k1 * g.W + k2];
                    }
                }
#pragma unroll
                for (int r = 0; r < R; r++) res[r] = combine<T, N>(v[r], s_tab, t[r].fx, t[r].fy, true, ~0u, ~0u);
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) res[r] = warp_interp_px<T, N>(img, g, t[r], sx[r], sy[r], ox, oys[r], s_tab);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++)
            if (y0 + r < y_end) out[(size_t)(y0 + r) * g.W + x] = res[r];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int rows_per_thread(int interp)
{
    return interp == MA_INTER_CUBIC ? Mode<MA_INTER_CUBIC>::R : interp == MA_INTER_LANCZOS4 ? Mode<MA_INTER_LANCZOS4>::R
                                                                                           : Mode<MA_INTER_NEAREST>::R;
}

// the warp kernel over output rows [y0, y1) of an (H, W) image on the ctx stream (interp: nearest / cubic / lanczos4)
int launch_warp(ma_ctx* ctx, const void* img, int dtype, const MaTiling& g, const float2* flow, void* out, int y0, int y1,
                int interp)
{
    const int R = rows_per_thread(interp);
    const int by = std::min((y1 - y0 + R - 1) / R, MA_GRID_Y_MAX);
    const dim3 grid((g.W + 255) / 256, by), block(256);
    const bool idx32 = (unsigned long long)g.H * (unsigned long long)g.W < (1ull << 31);
#define MA_WI(T, M) do { if (idx32) hipLaunchKernelGGL((warp_interp_kernel<T, M, true>), grid, block, 0, ctx->stream, (const T*)img, g, flow, (T*)out, y0, y1); \
                         else hipLaunchKernelGGL((warp_interp_kernel<T, M, false>), grid, block, 0, ctx->stream, (const T*)img, g, flow, (T*)out, y0, y1); } while (0)
#define MA_WI_T(T) do { if (interp == MA_INTER_NEAREST) MA_WI(T, MA_INTER_NEAREST); else if (interp == MA_INTER_CUBIC) MA_WI(T, MA_INTER_CUBIC); \
                        else MA_WI(T, MA_INTER_LANCZOS4); } while (0)
    if (dtype == MA_U8) MA_WI_T(uint8_t);
    else if (dtype == MA_U16) MA_WI_T(uint16_t);
    else MA_WI_T(float);
#undef MA_WI_T
#undef MA_WI
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" {

int ma_remap_interp(ma_ctx* ctx, const void* src, int dtype, int cn, int sh, int sw, const float* map_xy, int dh, int dw,
                    void* dst, int interp)
{
    MA_REQUIRE(interp_known(interp), "interp must be MA_INTER_NEAREST, _LINEAR, _CUBIC or _LANCZOS4");
    if (interp == MA_INTER_LINEAR) return ma_remap_bilinear(ctx, src, dtype, cn, sh, sw, map_xy, dh, dw, dst);
    MA_REQUIRE(ctx && src && map_xy && dst, "NULL argument");
    MA_REQUIRE_ALIGNED(map_xy, 8, "map_xy");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "dtype must be u8/u16/f32");
    MA_REQUIRE(cn >= 1 && cn <= 4, "cn must be 1 to 4");
    MA_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, "empty image");
    MA_REQUIRE(sh < 32767 && sw < 32767 && dh < 32767 && dw < 32767, "cv2.remap requires all dimensions < 32767");
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    MaProfScope ps(ctx, MA_K_OTHER, (double)dh * dw);
    const dim3 grid((dw + 255) / 256, dh), block(256);
    const float2* map = (const float2*)map_xy;
#define MA_RI(T, M, CN) hipLaunchKernelGGL((remap_interp_kernel<T, M, CN>), grid, block, 0, ctx->stream, (const T*)src, sh, sw, map, dh, dw, (T*)dst)
#define MA_RI_CN(T, M) do { if (cn == 1) MA_RI(T, M, 1); else if (cn == 2) MA_RI(T, M, 2); else if (cn == 3) MA_RI(T, M, 3); else MA_RI(T, M, 4); } while (0)
#define MA_RI_T(T) do { if (interp == MA_INTER_NEAREST) MA_RI_CN(T, MA_INTER_NEAREST); else if (interp == MA_INTER_CUBIC) MA_RI_CN(T, MA_INTER_CUBIC); \
                        else MA_RI_CN(T, MA_INTER_LANCZOS4); } while (0)
    if (dtype == MA_U8) MA_RI_T(uint8_t);
    else if (dtype == MA_U16) MA_RI_T(uint16_t);
    else MA_RI_T(float);
#undef MA_RI_T
#undef MA_RI_CN
#undef MA_RI
    MA_HIP(hipGetLastError());
    return MA_OK;
}

int ma_warp_tiled_interp(ma_ctx* ctx, const void* img, int dtype, int H, int W, const float* flow, int tile, int overlap,
                         void* out, int interp)
{
    MA_REQUIRE(interp_known(interp), "interp must be MA_INTER_NEAREST, _LINEAR, _CUBIC or _LANCZOS4");
    if (interp == MA_INTER_LINEAR) return ma_warp_tiled(ctx, img, dtype, H, W, flow, tile, overlap, out);
    MA_REQUIRE(ctx && img && flow && out, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "dtype must be u8/u16/f32");
    MA_REQUIRE(H > 0 && W > 0, "bad image size");
    MA_REQUIRE(tile >= 0 && overlap >= 0, "tile/overlap must be >= 0");
    const MaTiling g = ma_make_tiling(H, W, tile, overlap);
    MA_REQUIRE(g.Ph < 32767 && g.Pw < 32767, "cv2.remap requires window dimensions < 32767");
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    MaProfScope ps(ctx, MA_K_OTHER, (double)H * W);
    return launch_warp(ctx, img, dtype, g, (const float2*)flow, out, 0, H, interp);
}

// Page-warp driver with the interpolation modes: the bands and upload pieces of ma_warp_pages_host on the one pipeline
// (page_pipeline.hip), with this file's kernel on each band.
int ma_warp_pages_host_interp(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages, int dtype,
                              int H, int W, const float* flow, int tile, int overlap, int interp)
{
    MA_REQUIRE(interp_known(interp), "interp must be MA_INTER_NEAREST, _LINEAR, _CUBIC or _LANCZOS4");
    if (interp == MA_INTER_LINEAR) return ma_warp_pages_host(ctx, pages_host, out_host, n_pages, dtype, H, W, flow, tile, overlap);
    MA_REQUIRE(ctx && pages_host && out_host && flow, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "dtype must be u8/u16/f32");
    MA_REQUIRE(n_pages >= 0, "bad page count");
    long long band_bytes = 0;
    MA_TRY(ma_ctx_get_option(ctx, MA_OPT_WARP_BAND_BYTES, &band_bytes));
    MaPagePlan plan;
    MA_TRY(ma_warp_pages_tiled_plan(dtype, H, W, tile, overlap, (size_t)band_bytes, &plan));
    const MaTiling g = ma_make_tiling(H, W, tile, overlap);
    MA_REQUIRE(g.Ph < 32767 && g.Pw < 32767, "cv2.remap requires window dimensions < 32767");
    for (int i = 0; i < n_pages; i++) MA_REQUIRE(pages_host[i] && out_host[i], "NULL page pointer");
    if (n_pages == 0) return MA_OK;
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    return ma_warp_pages_run(ctx, pages_host, out_host, n_pages, plan, [&](const void* din, void* dout, int y0, int y1) {
        return launch_warp(ctx, din, dtype, g, (const float2*)flow, dout, y0, y1, interp);
    });
}

} // extern "C"
