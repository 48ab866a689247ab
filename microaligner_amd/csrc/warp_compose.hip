// One resampling through a 2 x 3 affine initialisation and a flow (include/microaligner_compose.h): the moving image is
// sampled once, at float32(M.(p - flow(p))), instead of transform_img_with_tmat's warp followed by Warper.warp()'s.
// Off the measured path.
//
// The map is evaluated in float64 with every multiply and add rounded on its own (__dmul_rn / __dadd_rn), so that a plain
// numpy float64 statement reproduces it bit for bit.  The sample is cv2.remap's on the zero-padded (H, W) source, which is
// never built: a tap reads the (h, w) image at (sx - left, sy - top) and 0 outside it.  Nearest, cubic and Lanczos-4 take
// their taps and weights from remap_interp.h (shared with remap_interp.hip); the linear sample restates remap.hip's.
//
// A block covers a 2-D tile of the output, 64 columns by 4 waves x R rows, so that the source footprint stays compact when
// the matrix rotates; a thread takes R rows of one column and, when every tap of its wave lies inside the image, issues all
// their loads before the first sum.
#include "remap_interp.h"
#include "../../include/microaligner_compose.h"

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <string>
#include <thread>

namespace {

// ---- the linear sample ----------------------------------------------------------------------------------------------
// remap.hip's weights_i / weights_f / Interp<T> (cv2.remap INTER_LINEAR), restated here rather
// than shared: remap.hip is on the measured path and under build.source_hash(), and stays as the measured path has it
// (remap_interp.hip restates its window origins for the same reason).

// 15-bit fixed-point bilinear weights of OpenCV's BilinearTab_i, including the [32767,0,0,1] entry that the table's sum
// fix-up produces at zero fraction
__device__ __forceinline__ void lin_weights_i(int fx, int fy, int w[4])
{
    if ((fx | fy) == 0) { w[0] = 32767; w[1] = 0; w[2] = 0; w[3] = 1; return; }
    w[0] = (32 - fy) * (32 - fx) * 32; w[1] = (32 - fy) * fx * 32;
    w[2] = fy * (32 - fx) * 32;        w[3] = fy * fx * 32;
}
__device__ __forceinline__ void lin_weights_f(int fx, int fy, float w[4])
{
    // products of the exact 1-D weights (1 - f/32, f/32): exact in float
    const float s = 1.f / 32.f;
    float x1 = fx * s, x0 = 1.f - x1, y1 = fy * s, y0 = 1.f - y1;
    w[0] = y0 * x0; w[1] = y0 * x1; w[2] = y1 * x0; w[3] = y1 * x1;
}
// the four taps (top left, top right, bottom left, bottom right) summed in that order; taps outside the source hold 0
template <typename T>
__device__ __forceinline__ T lin_sample(const T (&v)[2][2], int fx, int fy)
{
    if constexpr (sizeof(T) == 1) {
        int w[4];
        lin_weights_i(fx, fy, w);
        const int acc = v[0][0] * w[0] + v[0][1] * w[1] + v[1][0] * w[2] + v[1][1] * w[3];
        return (T)d_clamp((acc + (1 << 14)) >> 15, 0, 255);
    } else {
        float w[4];
        lin_weights_f(fx, fy, w);
        const float acc = (float)v[0][0] * w[0] + (float)v[0][1] * w[1] + (float)v[1][0] * w[2] + (float)v[1][1] * w[3];
        if constexpr (sizeof(T) == 2) return (T)d_clamp(d_cvround(acc), 0, 65535);
        else return acc;
    }
}

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

// remap_interp.h's quantise() without the saturation of the integer part to 16 bits: sides of 32767 px and more work.
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
        return lin_sample<T>(v, t.fx, t.fy);
    } else {
        const bool fast = d_below(sx, a.W - N + 1) && d_below(sy, a.H - N + 1);
        return combine<T, N>(v, s_tab, t.fx, t.fy, fast, rmask, cmask);
    }
}

// Output rows [y_begin, y_end) (the whole image for ma_warp_affine_flow, one band for the page driver).  Block tiles beyond
// the grid's y extent loop (gridDim.y is capped).  IDX32: the output has fewer than 2^31 elements (so has the image).
template <typename T, int MODE, bool IDX32>
__global__ __launch_bounds__(256) void warp_compose_kernel(const T* __restrict__ img, ComposeArgs a,
                                                           const float2* __restrict__ flow, T* __restrict__ out,
                                                           int y_begin, int y_end)
{
    constexpr int N = Compose<MODE>::N, OFF = Compose<MODE>::OFF, R = Compose<MODE>::R, TILE_H = WAVES * R;
    __shared__ float s_tab[TAB * (N > 2 ? N : 1)];
    if constexpr (N > 2) load_tab<N>(s_tab);
    const int x = blockIdx.x * TILE_W + (int)(threadIdx.x & 63);
    const int wave = (int)(threadIdx.x >> 6);
    if (x >= a.W) return;
    for (int yt = y_begin + (int)blockIdx.y * TILE_H; yt < y_end; yt += (int)gridDim.y * TILE_H) {
        const int y0 = yt + wave * R;
        if (y0 >= y_end) continue;   // wave-uniform
        float2 f[R];
        int ys[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            ys[r] = min(y0 + r, y_end - 1);
            f[r] = IDX32 ? flow[(unsigned)ys[r] * (unsigned)a.W + (unsigned)x] : flow[(size_t)ys[r] * a.W + x];
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
                    if constexpr (MODE == MA_INTER_LINEAR) res[r] = lin_sample<T>(v[r], t[r].fx, t[r].fy);
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

// the kernel over output rows [y0, y1) on the ctx stream
int launch_compose(ma_ctx* ctx, const void* img, int dtype, const ComposeArgs& a, const float2* flow, void* out, int y0,
                   int y1, int interp)
{
    const int th = WAVES * compose_rows(interp);
    const dim3 grid((a.W + TILE_W - 1) / TILE_W, std::min((y1 - y0 + th - 1) / th, MA_GRID_Y_MAX)), block(256);
    const bool idx32 = (unsigned long long)a.H * (unsigned long long)a.W < (1ull << 31);
#define MA_WC(T, M) do { if (idx32) hipLaunchKernelGGL((warp_compose_kernel<T, M, true>), grid, block, 0, ctx->stream, (const T*)img, a, flow, (T*)out, y0, y1); \
                         else hipLaunchKernelGGL((warp_compose_kernel<T, M, false>), grid, block, 0, ctx->stream, (const T*)img, a, flow, (T*)out, y0, y1); } while (0)
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
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    MaProfScope ps(ctx, MA_K_OTHER, (double)H * W);
    return launch_compose(ctx, img, dtype, make_args(h, w, pad_left, pad_top, H, W, m), (const float2*)flow, out, 0, H,
                          interp);
}

// Page driver: ma_warp_pages_host_interp's pipeline on the three engines with NS slots, except that a page goes up whole
// (without a pass over the flow the source rows an output band reads are not bounded) and only the output is cut into
// bands.  An upload thread copies page i into input slot i % NS on the H2D engine while this thread launches the bands of
// page i - 1 on the compute engine, and a download thread copies each band's output rows out on the D2H engine as soon as
// its kernel has run; events order the engines, counters under one mutex order the threads.
int ma_warp_affine_flow_pages_host(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages,
                                   int dtype, int h, int w, int pad_left, int pad_top, const float* flow, int H, int W,
                                   const double m[6], int interp)
{
    MA_TRY(check_args(dtype, h, w, pad_left, pad_top, H, W, m, interp));
    MA_REQUIRE(ctx && pages_host && out_host && flow, "NULL argument");
    MA_REQUIRE(n_pages >= 0, "bad page count");
    for (int i = 0; i < n_pages; i++) MA_REQUIRE(pages_host[i] && out_host[i], "NULL page pointer");
    if (n_pages == 0) return MA_OK;
    long long band_bytes = 0;
    MA_TRY(ma_ctx_get_option(ctx, MA_OPT_WARP_BAND_BYTES, &band_bytes));
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ensure_tables(ctx));
    const ComposeArgs args = make_args(h, w, pad_left, pad_top, H, W, m);

    constexpr int NS = 3;
    const int ns = n_pages < NS ? n_pages : NS;
    const size_t es = ma_esize(dtype), rowb = (size_t)W * es, nb_in = (size_t)h * w * es, nb_out = (size_t)H * rowb;
    const int band_rows = (int)std::min<size_t>((size_t)H, std::max<size_t>(1, ((size_t)band_bytes + rowb - 1) / rowb));
    const int nband = (H + band_rows - 1) / band_rows;
    const size_t in_bytes = ma_align_up(nb_in, 256), out_bytes = ma_align_up(nb_out, 256);
    MA_TRY(ma_ws_reserve(ctx, (in_bytes + out_bytes) * ns));   // device slots in the context workspace
    char *din[NS], *dout[NS];
    for (int k = 0; k < ns; k++) {
        din[k] = (char*)ctx->ws + (in_bytes + out_bytes) * k;
        dout[k] = din[k] + in_bytes;
    }
    std::vector<void*> ev_up((size_t)ns, nullptr), ev_k((size_t)ns * nband, nullptr);
    void* ws_idle = nullptr;
    auto cleanup = [&]() {
        for (void* e : ev_up) if (e) (void)ma_event_destroy(ctx, e);
        for (void* e : ev_k) if (e) (void)ma_event_destroy(ctx, e);
        if (ws_idle) (void)ma_event_destroy(ctx, ws_idle);
    };
    int rc = ma_event_create(ctx, &ws_idle);
    for (size_t e = 0; rc == MA_OK && e < ev_up.size(); e++) rc = ma_event_create(ctx, &ev_up[e]);
    for (size_t e = 0; rc == MA_OK && e < ev_k.size(); e++) rc = ma_event_create(ctx, &ev_k[e]);
    // the slots may still be in use by kernels enqueued earlier on the compute stream: both transfer engines start behind
    // everything it holds now
    if (rc == MA_OK) rc = ma_engine_record(ctx, MA_ENGINE_COMPUTE, ws_idle);
    if (rc == MA_OK) rc = ma_engine_wait(ctx, MA_ENGINE_H2D, ws_idle);
    if (rc == MA_OK) rc = ma_engine_wait(ctx, MA_ENGINE_D2H, ws_idle);
    if (rc != MA_OK) {
        cleanup();
        return rc;
    }
    auto band_begin = [&](int b) { return b * band_rows; };
    auto band_end = [&](int b) { return std::min(H, (b + 1) * band_rows); };
    std::vector<size_t> cuts_out(nband);
    for (int b = 0; b < nband; b++) cuts_out[b] = (size_t)band_end(b) * rowb;

    std::mutex mu;
    std::condition_variable cv;
    int uploaded = 0, downloaded = 0;   // in pages
    long long launched = 0;             // in units (page * nband + band)
    int failed = MA_OK;
    std::string what;
    auto fail = [&](int r) {   // called with mu held
        if (failed == MA_OK) { failed = r; what = ma_last_error(); }
        cv.notify_all();
    };
    std::thread up([&]() {
        for (int i = 0; i < n_pages; i++) {
            const int k = i % ns;
            {   // slot k is free again once page i - ns has been downloaded
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return failed != MA_OK || downloaded > i - ns; });
                if (failed != MA_OK) return;
            }
            const int r = ma_engine_h2d_pieces(ctx, MA_ENGINE_H2D, din[k], pages_host[i], nb_in, &nb_in, 1, [&](int) {
                const int rr = ma_engine_record(ctx, MA_ENGINE_H2D, ev_up[k]);
                std::lock_guard<std::mutex> lk(mu);
                if (rr != MA_OK) return rr;
                if (failed != MA_OK) return failed;
                uploaded = i + 1;
                cv.notify_all();
                return (int)MA_OK;
            }, false);   // no wait at the page boundary: the next page's first chunk is staged under this page's last DMAs
            if (r != MA_OK) {
                std::lock_guard<std::mutex> lk(mu);
                fail(r);
                return;
            }
        }
        const int r = ma_engine_sync(ctx, MA_ENGINE_H2D);
        if (r != MA_OK) {
            std::lock_guard<std::mutex> lk(mu);
            fail(r);
        }
    });
    std::thread down([&]() {
        for (int i = 0; i < n_pages; i++) {
            const int k = i % ns;
            const int r = ma_engine_d2h_pieces(ctx, MA_ENGINE_D2H, out_host[i], dout[k], nb_out, cuts_out.data(), nband, [&](int b) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return failed != MA_OK || launched > (long long)i * nband + b; });
                    if (failed != MA_OK) return failed;
                }
                return ma_engine_wait(ctx, MA_ENGINE_D2H, ev_k[(size_t)k * nband + b]);
            });
            std::lock_guard<std::mutex> lk(mu);
            if (r != MA_OK) { fail(r); return; }
            downloaded = i + 1;
            cv.notify_all();
        }
    });
    for (int i = 0; i < n_pages; i++) {
        const int k = i % ns;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return failed != MA_OK || uploaded > i; });
            if (failed != MA_OK) break;
        }
        int r = ma_engine_wait(ctx, MA_ENGINE_COMPUTE, ev_up[k]);
        for (int b = 0; r == MA_OK && b < nband; b++) {
            r = launch_compose(ctx, din[k], dtype, args, (const float2*)flow, dout[k], band_begin(b), band_end(b), interp);
            if (r == MA_OK) r = ma_engine_record(ctx, MA_ENGINE_COMPUTE, ev_k[(size_t)k * nband + b]);
            if (r == MA_OK) {
                std::lock_guard<std::mutex> lk(mu);
                launched = (long long)i * nband + b + 1;
                cv.notify_all();
            }
        }
        if (r != MA_OK) {
            std::lock_guard<std::mutex> lk(mu);
            fail(r);
            break;
        }
    }
    up.join();
    down.join();
    // also when a thread gave up early: nothing of this call may still be reading the caller's pages or writing its
    // results once it has returned
    (void)ma_engine_sync(ctx, MA_ENGINE_H2D);
    (void)ma_engine_sync(ctx, MA_ENGINE_D2H);
    (void)hipStreamSynchronize(ctx->stream);
    cleanup();
    if (failed != MA_OK) {
        ma_set_error("%s", what.c_str());
        return failed;
    }
    return MA_OK;
}

} // extern "C"
