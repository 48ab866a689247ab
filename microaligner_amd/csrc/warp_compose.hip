// One resampling through a 2 x 3 affine initialisation and a flow (include/microaligner_compose.h): the moving image is
// sampled once, at float32(M.(p - flow(p))), instead of transform_img_with_tmat's warp followed by Warper.warp()'s.
// Off the measured path.
//
// The map is evaluated in float64 with every multiply and add rounded on its own (__dmul_rn / __dadd_rn), so that a plain
// numpy float64 statement reproduces it bit for bit.  The sample is cv2.remap's on the zero-padded (H, W) source, which is
// never built: a tap reads the (h, w) image at (sx - left, sy - top) and 0 outside it.  Nearest, cubic and Lanczos-4 take
// their taps and weights from remap_interp.h (shared with remap_interp.hip), linear takes remap_common.h's bilinear sample.
//
// A block covers a 2-D tile of the output, 64 columns by 4 waves x R rows, so that the source footprint stays compact when
// the matrix rotates; a thread takes R rows of one column and, when every tap of its wave lies inside the image, issues all
// their loads before the first sum.
//
// The flow of a pixel comes from one of two sources (the kernel's SRC): the dense array, or the nodes of a grid flow
// (include/microaligner_flowgrid.h), evaluated from the block's node patch in LDS (flow_grid_eval.h); everything after
// f[r] is the same code, so the warp from a grid is the dense warp of the expanded flow bit for bit.
#include "remap_interp.h"
#include "flow_grid_eval.h"
#include "../../include/microaligner_compose.h"
#include "../../include/microaligner_flowgrid.h"

#include <algorithm>

namespace {

// ---- the map --------------------------------------------------------------------------------------------------------
struct ComposeArgs {
    double m[6];      // rows 0-1 of M = pinv([T; 0 0 1]), row-major
    int h, w;         // the moving image
    int left, top;    // its offset in the padded (H, W) source
    int H, W;         // the output, the flow and the padded source
};

// float32((m0 qx + m1 qy) + m2) with q = p - flow(p), every operation rounded in float64 on its own
__device__ __forceinline__ float2 compose_map(const ComposeArgs& a, int x, int y, float2 f)
{
    const double qx = __dadd_rn((double)x, -(double)f.x), qy = __dadd_rn((double)y, -(double)f.y);
    return make_float2((float)__dadd_rn(__dadd_rn(__dmul_rn(a.m[0], qx), __dmul_rn(a.m[1], qy)), a.m[2]),
                       (float)__dadd_rn(__dadd_rn(__dmul_rn(a.m[3], qx), __dmul_rn(a.m[4], qy)), a.m[5]));
}

// remap_common.h's quantise() without the saturation of the integer part to 16 bits: sides of 32767 px and more work.
// A coordinate that cvRound sends to INT_MIN lands at -2^26, far outside any source.
__device__ __forceinline__ Tap quantise_wide(float2 m)
{
    const int sxq = d_cvround(m.x * 32.f), syq = d_cvround(m.y * 32.f);
    Tap t;
    t.fx = sxq & 31; t.fy = syq & 31;
    t.sx = sxq >> 5; t.sy = syq >> 5;
    return t;
}

// taps per side N, offset of the first tap OFF, output rows per thread R
template <int MODE> struct Compose;
template <> struct Compose<MA_INTER_NEAREST> { static constexpr int N = 1, OFF = 0, R = 8; };
template <> struct Compose<MA_INTER_LINEAR> { static constexpr int N = 2, OFF = 0, R = 8; };
template <> struct Compose<MA_INTER_CUBIC> { static constexpr int N = 4, OFF = 1, R = 4; };
template <> struct Compose<MA_INTER_LANCZOS4> { static constexpr int N = 8, OFF = 3, R = 2; };

constexpr int TILE_W = 64, WAVES = 4;

// one sample whose top-left tap (sx, sy) is in padded coordinates: taps outside the padded source are skipped by the sum
// unless every tap is inside it, taps in the padding read 0
template <typename T, int MODE>
__device__ __forceinline__ T compose_px(const T* __restrict__ img, const ComposeArgs& a, const Tap& t, int sx, int sy,
                                        const float* s_tab)
{
    constexpr int N = Compose<MODE>::N;
    if (sx >= a.W || sx + N <= 0 || sy >= a.H || sy + N <= 0) return (T)0;
    unsigned rmask = 0, cmask = 0, rimg = 0, cimg = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
        rmask |= (unsigned)((unsigned)(sy + k) < (unsigned)a.H) << k;
        cmask |= (unsigned)((unsigned)(sx + k) < (unsigned)a.W) << k;
        rimg |= (unsigned)((unsigned)(sy + k - a.top) < (unsigned)a.h) << k;
        cimg |= (unsigned)((unsigned)(sx + k - a.left) < (unsigned)a.w) << k;
    }
    T v[N][N];
#pragma unroll
    for (int k1 = 0; k1 < N; k1++)
#pragma unroll
        for (int k2 = 0; k2 < N; k2++)
            v[k1][k2] = ((rimg >> k1) & (cimg >> k2) & 1u) ? img[(size_t)(sy + k1 - a.top) * a.w + (sx + k2 - a.left)] : (T)0;
    if constexpr (MODE == MA_INTER_LINEAR) {
        return Interp<T>::run(v[0][0], v[0][1], v[1][0], v[1][1], t.fx, t.fy);
    } else {
        const bool fast = d_below(sx, a.W - N + 1) && d_below(sy, a.H - N + 1);
        return combine<T, N>(v, s_tab, t.fx, t.fy, fast, rmask, cmask);
    }
}

// the two sources of a pixel's flow
struct DenseFlow { const float2* __restrict__ p; };   // (H, W)
struct GridFlow { FgGrid g; };

// Output rows [y_begin, y_end) (the whole image for ma_warp_affine_flow, one band for the page driver).  Block tiles beyond
// the grid's y extent loop (gridDim.y is capped).  IDX32: the output has fewer than 2^31 elements (so has the image).
template <typename T, int MODE, bool IDX32, class SRC>
__global__ __launch_bounds__(256) void warp_compose_kernel(const T* __restrict__ img, ComposeArgs a, SRC src,
                                                           T* __restrict__ out, int y_begin, int y_end)
{
    constexpr int N = Compose<MODE>::N, OFF = Compose<MODE>::OFF, R = Compose<MODE>::R, TILE_H = WAVES * R;
    constexpr bool GRID = std::is_same<SRC, GridFlow>::value;
    static_assert(TILE_W == FG_TILE_W, "the node patch is as wide as the tile");
    __shared__ float s_tab[TAB * (N > 2 ? N : 1)];
    if constexpr (N > 2) load_tab<N>(s_tab);
    const int x = blockIdx.x * TILE_W + (int)(threadIdx.x & 63);
    const int wave = (int)(threadIdx.x >> 6);
    // with a grid every thread of the block stages the tile's nodes, so none leaves before the barriers
    if constexpr (!GRID)
        if (x >= a.W) return;
    for (int yt = y_begin + (int)blockIdx.y * TILE_H; yt < y_end; yt += (int)gridDim.y * TILE_H) {
        const int y0 = yt + wave * R;
        float2 f[R];
        int ys[R];
        if constexpr (GRID) {
            __shared__ FgTile<TILE_H> s_tile;
            const int bx0 = blockIdx.x * TILE_W;
            __syncthreads();      // the tile before is read
            fg_stage(s_tile, src.g, bx0, min(bx0 + TILE_W, a.W), yt, min(yt + TILE_H, y_end), (int)threadIdx.x, 256);
            __syncthreads();
            if (x >= a.W || y0 >= y_end) continue;
            const FgCol col = fg_col(src.g, bx0, x);
#pragma unroll
            for (int r = 0; r < R; r++) {
                ys[r] = min(y0 + r, y_end - 1);
                f[r] = fg_eval(s_tile, src.g, col, ys[r] - yt);
            }
        } else {
            if (y0 >= y_end) continue;   // wave-uniform
#pragma unroll
            for (int r = 0; r < R; r++) {
                ys[r] = min(y0 + r, y_end - 1);
                f[r] = IDX32 ? src.p[(unsigned)ys[r] * (unsigned)a.W + (unsigned)x] : src.p[(size_t)ys[r] * a.W + x];
            }
        }
        T res[R];
        if constexpr (MODE == MA_INTER_NEAREST) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float2 m = compose_map(a, x, ys[r], f[r]);
                // unsigned differences: a coordinate of INT_MIN (non-finite map) wraps far beyond the image
                const unsigned ix = (unsigned)d_cvround(m.x) - (unsigned)a.left, iy = (unsigned)d_cvround(m.y) - (unsigned)a.top;
                res[r] = (ix < (unsigned)a.w && iy < (unsigned)a.h) ? img[(size_t)iy * a.w + ix] : (T)0;
            }
        } else {
            Tap t[R];
            int sx[R], sy[R];
            bool inside = true;
#pragma unroll
            for (int r = 0; r < R; r++) {
                t[r] = quantise_wide(compose_map(a, x, ys[r], f[r]));
                sx[r] = t[r].sx - OFF; sy[r] = t[r].sy - OFF;
                inside = inside && d_below(sx[r] - a.left, a.w - N + 1) && d_below(sy[r] - a.top, a.h - N + 1);
            }
            if (__all(inside)) {
                // every tap of every row of the wave inside the image: OpenCV's straight path, loads first
                T v[R][N][N];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if (IDX32) {
                        const unsigned p = (unsigned)(sy[r] - a.top) * (unsigned)a.w + (unsigned)(sx[r] - a.left);
#pragma unroll
                        for (int k1 = 0; k1 < N; k1++)
#pragma unroll
                            for (int k2 = 0; k2 < N; k2++) v[r][k1][k2] = img[p + (unsigned)k1 * (unsigned)a.w + (unsigned)k2];
                    } else {
                        const T* q = img + (size_t)(sy[r] - a.top) * a.w + (sx[r] - a.left);
#pragma unroll
                        for (int k1 = 0; k1 < N; k1++)
#pragma unroll
                            for (int k2 = 0; k2 < N; k2++) v[r][k1][k2] = q[(size_t)k1 * a.w + k2];
                    }
                }
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if constexpr (MODE == MA_INTER_LINEAR)
                        res[r] = Interp<T>::run(v[r][0][0], v[r][0][1], v[r][1][0], v[r][1][1], t[r].fx, t[r].fy);
                    else res[r] = combine<T, N>(v[r], s_tab, t[r].fx, t[r].fy, true, ~0u, ~0u);
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) res[r] = compose_px<T, MODE>(img, a, t[r], sx[r], sy[r], s_tab);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (y0 + r < y_end) {
                if (IDX32) out[(unsigned)(y0 + r) * (unsigned)a.W + (unsigned)x] = res[r];
                else out[(size_t)(y0 + r) * a.W + x] = res[r];
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int compose_rows(int interp)
{
    return interp == MA_INTER_NEAREST ? Compose<MA_INTER_NEAREST>::R : interp == MA_INTER_LINEAR ? Compose<MA_INTER_LINEAR>::R
         : interp == MA_INTER_CUBIC ? Compose<MA_INTER_CUBIC>::R : Compose<MA_INTER_LANCZOS4>::R;
}

int check_args(int dtype, int h, int w, int pad_left, int pad_top, int H, int W, const double* m, int interp)
{
    MA_REQUIRE(interp_known(interp), "interp must be MA_INTER_NEAREST, _LINEAR, _CUBIC or _LANCZOS4");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "dtype must be u8/u16/f32");
    MA_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0, "empty image");
    MA_REQUIRE(h <= H && w <= W, "the image must be no larger than the flow in either dimension");
    // keeps every tap coordinate minus the padding inside int
    MA_REQUIRE(H <= (1 << 30) && W <= (1 << 30), "sides must be at most 2^30");
    MA_REQUIRE(pad_left >= 0 && pad_top >= 0 && pad_left <= W - w && pad_top <= H - h,
               "the padding must place the image inside the flow's shape");
    MA_REQUIRE(m, "NULL matrix");
    for (int i = 0; i < 6; i++) MA_REQUIRE(std::isfinite(m[i]), "the matrix must be finite");
    return MA_OK;
}

ComposeArgs make_args(int h, int w, int pad_left, int pad_top, int H, int W, const double* m)
{
    ComposeArgs a;
    for (int i = 0; i < 6; i++) a.m[i] = m[i];
    a.h = h; a.w = w; a.left = pad_left; a.top = pad_top; a.H = H; a.W = W;
    return a;
}

// the kernel over output rows [y0, y1) on the ctx stream, the flow from `src`
template <class SRC>
int launch_compose(ma_ctx* ctx, const void* img, int dtype, const ComposeArgs& a, const SRC& src, void* out, int y0,
                   int y1, int interp)
{
    const int th = WAVES * compose_rows(interp);
    const dim3 grid((a.W + TILE_W - 1) / TILE_W, std::min((y1 - y0 + th - 1) / th, MA_GRID_Y_MAX)), block(256);
    const bool idx32 = (unsigned long long)a.H * (unsigned long long)a.W < (1ull << 31);
#define MA_WC(T, M) do { if (idx32) hipLaunchKernelGGL((warp_compose_kernel<T, M, true, SRC>), grid, block, 0, ctx->stream, (const T*)img, a, src, (T*)out, y0, y1); \
                         else hipLaunchKernelGGL((warp_compose_kernel<T, M, false, SRC>), grid, block, 0, ctx->stream, (const T*)img, a, src, (T*)out, y0, y1); } while (0)
#define MA_WC_T(T) do { if (interp == MA_INTER_NEAREST) MA_WC(T, MA_INTER_NEAREST); else if (interp == MA_INTER_LINEAR) MA_WC(T, MA_INTER_LINEAR); \
                        else if (interp == MA_INTER_CUBIC) MA_WC(T, MA_INTER_CUBIC); else MA_WC(T, MA_INTER_LANCZOS4); } while (0)
    if (dtype == MA_U8) MA_WC_T(uint8_t);
    else if (dtype == MA_U16) MA_WC_T(uint16_t);
    else MA_WC_T(float);
#undef MA_WC_T
#undef MA_WC
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // namespace

extern "C" {

int ma_warp_affine_flow(ma_ctx* ctx, const void* img, int dtype, int h, int w, int pad_left, int pad_top,
                        const float* flow, int H, int W, const double m[6], void* out, int interp)
{
    MA_TRY(check_args(dtype, h, w, pad_left, pad_top, H, W, m, interp));
    MA_REQUIRE(ctx && img && flow && out, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    MaProfScope ps(ctx, MA_K_OTHER, (double)H * W);
    return launch_compose(ctx, img, dtype, make_args(h, w, pad_left, pad_top, H, W, m), DenseFlow{(const float2*)flow}, out,
                          0, H, interp);
}

int ma_warp_affine_grid(ma_ctx* ctx, const void* img, int dtype, int h, int w, int pad_left, int pad_top,
                        const float* nodes, int H, int W, int s, const double m[6], void* out, int interp)
{
    MA_TRY(check_args(dtype, h, w, pad_left, pad_top, H, W, m, interp));
    MA_REQUIRE(ctx && img && nodes && out, "NULL argument");
    MA_REQUIRE_ALIGNED(nodes, 8, "nodes");
    MA_REQUIRE(s >= 1, "the stride must be at least 1");
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    MaProfScope ps(ctx, MA_K_OTHER, (double)H * W);
    return launch_compose(ctx, img, dtype, make_args(h, w, pad_left, pad_top, H, W, m), GridFlow{fg_grid(nodes, H, W, s)}, out,
                          0, H, interp);
}

} // extern "C"

namespace {

// Page driver: the one pipeline (page_pipeline.hip), except that a page goes up whole (without a pass over the flow the
// source rows an output band reads are not bounded) and only the output is cut into bands, of MA_OPT_WARP_BAND_BYTES and
// no tile alignment: page i goes up while the bands of page i - 1 are launched, and each band's rows come down as soon as
// its kernel has run.
template <class SRC>
int compose_pages(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages, int dtype, int h, int w,
                  int pad_left, int pad_top, const SRC& src, int H, int W, const double m[6], int interp)
{
    MA_TRY(check_args(dtype, h, w, pad_left, pad_top, H, W, m, interp));
    MA_REQUIRE(ctx && pages_host && out_host, "NULL argument");
    MA_REQUIRE(n_pages >= 0, "bad page count");
    for (int i = 0; i < n_pages; i++) MA_REQUIRE(pages_host[i] && out_host[i], "NULL page pointer");
    if (n_pages == 0) return MA_OK;
    long long band_bytes = 0;
    MA_TRY(ma_ctx_get_option(ctx, MA_OPT_WARP_BAND_BYTES, &band_bytes));
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    const ComposeArgs args = make_args(h, w, pad_left, pad_top, H, W, m);
    const size_t rowb = (size_t)W * ma_esize(dtype);
    const int band_rows = (int)std::min<size_t>((size_t)H, std::max<size_t>(1, ((size_t)band_bytes + rowb - 1) / rowb));
    MaPagePlan plan;
    plan.in_bytes = (size_t)h * w * ma_esize(dtype);
    plan.out_bytes = (size_t)H * rowb;
    plan.out_row_bytes = rowb;
    plan.cuts_src.assign(1, plan.in_bytes);
    for (int y = 0; y < H; y += band_rows) plan.cuts_out.push_back((size_t)std::min(H, y + band_rows) * rowb);
    return ma_warp_pages_run(ctx, pages_host, out_host, n_pages, plan, [&](const void* din, void* dout, int y0, int y1) {
        return launch_compose(ctx, din, dtype, args, src, dout, y0, y1, interp);
    });
}

} // namespace

extern "C" {

int ma_warp_affine_flow_pages_host(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages,
                                   int dtype, int h, int w, int pad_left, int pad_top, const float* flow, int H, int W,
                                   const double m[6], int interp)
{
    MA_REQUIRE(flow, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    return compose_pages(ctx, pages_host, out_host, n_pages, dtype, h, w, pad_left, pad_top, DenseFlow{(const float2*)flow}, H,
                         W, m, interp);
}

int ma_warp_affine_grid_pages_host(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages,
                                   int dtype, int h, int w, int pad_left, int pad_top, const float* nodes, int H, int W,
                                   int s, const double m[6], int interp)
{
    MA_REQUIRE(nodes, "NULL argument");
    MA_REQUIRE_ALIGNED(nodes, 8, "nodes");
    MA_REQUIRE(s >= 1, "the stride must be at least 1");
    MA_REQUIRE(H > 0 && W > 0, "empty image");
    return compose_pages(ctx, pages_host, out_host, n_pages, dtype, h, w, pad_left, pad_top,
                         GridFlow{fg_grid(nodes, H, W, s)}, H, W, m, interp);
}

} // extern "C"
