// Median filter of a flow and its outlier mask (include/microaligner_flowmedian.h).  Off the measured path: nothing in
// register() or warp() calls it.
//
// One kernel per call.  A block of 256 threads owns a tile of MF_TH x MF_TW pixels: it stages the tile and an r halo once
// into LDS as the header's int32 keys, an (u, v) pair per pixel (coalesced float2 loads, the weight looked up beside them),
// a sample that does not participate or lies outside the image as the marker MF_MARK in both components.  Lane = column,
// a wave owns MF_TH / 4 rows; a thread selects both components of a pixel as two independent chains, then writes out, keep
// and its share of the counts (call_counts.h).  No scratch, no workspace but the counters.
//   - generic (R = 0), every r in 1 .. 7 and every n: one sweep of the window for n and the smallest and largest key, then
//     bisection on the key between those two, counting the keys <= pivot over the window, until the smallest key with
//     (n - 1) / 2 + 1 keys at or below it is left -- a key of the window, so the result is exact.  The marker is above
//     every pivot and is never counted.
//   - registers (R = 1, 2, 3): the 9, 25 or 49 keys of a component live in registers.  Missing samples become balanced
//     sentinels (mf_window_registers), and a forgetful selection of min / max exchanges leaves the rank (N - 1) / 2
//     of the padded set, which is rank (n - 1) / 2 of the real keys.
// Both work on the integer keys: the result does not depend on how float min / max treat +-0 and denormals, and the
// selection compiles to v_min_i32 / v_max_i32 / v_med3_i32.
#include "../../include/microaligner_flowmedian.h"
#include "call_counts.h"
#include "weight_map.h"

#include <climits>
#include <cmath>

namespace {

constexpr int MF_SIDE_MAX = 1 << 24;
constexpr int MF_TW = 64, MF_TH = 32, MF_ROWS = MF_TH / 4;   // the tile, and the rows of a wave (= pixels of a thread)
constexpr int MF_REG_MAX_RADIUS = 3;                         // the largest radius of the register path
constexpr int MF_MARK = INT_MAX;                             // the key of a NaN: no participating value has it

// the header's key of a float's bits, and back (the map is its own inverse)
__device__ __forceinline__ int mf_key(float v)
{
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float mf_value(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

__device__ __forceinline__ int mf_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int mf_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ void mf_cswap(int& a, int& b)
{
    const int lo = mf_min(a, b), hi = mf_max(a, b);
    a = lo;
    b = hi;
}

// a[0 .. M): the smallest value to a[0], the largest to a[M - 1], the multiset kept.  Pairs from the two ends first, so
// that the smallest is in the lower half and the largest in the upper (the middle of an odd M belongs to both).
template <int M>
__device__ __forceinline__ void mf_minmax(int* a)
{
#pragma unroll
    for (int i = 0; i < M / 2; i++) mf_cswap(a[i], a[M - 1 - i]);
#pragma unroll
    for (int i = 1; i < (M + 1) / 2; i++) mf_cswap(a[0], a[i]);
#pragma unroll
    for (int i = M / 2; i < M - 1; i++) mf_cswap(a[i], a[M - 1]);
}

// Forgetful selection of the rank (N - 1) / 2 of k[0 .. N), N odd; k is destroyed.  Among N' values whose median is
// wanted, neither the smallest nor the largest of any N' / 2 + 2 of them can be it: drop both, take in one more value,
// and the median of the N' - 2 that are left is the same.  M = the working set, k[M0 - M .. M0); the next value enters
// in the place of the dropped largest.  Ends at three values, in a v_med3_i32.
template <int N, int M>
__device__ __forceinline__ int mf_forget(int* k)
{
    constexpr int M0 = N / 2 + 2, off = M0 - M;
    if constexpr (M == 3) {
        return mf_max(mf_min(k[off], k[off + 1]), mf_min(mf_max(k[off], k[off + 1]), k[off + 2]));
    } else {
        mf_minmax<M>(k + off);
        k[M0 - 1] = k[M0 + off];
        return mf_forget<N, M - 1>(k);
    }
}

template <int N>
__device__ __forceinline__ int mf_select(int* k)
{
    return mf_forget<N, N / 2 + 2>(k);
}

// Register path.  base: the window's first sample in the tile.  Missing samples (markers) become balanced sentinels: with
// n real keys among N, the first (N - 1) / 2 - (n - 1) / 2 of them INT_MIN and the others INT_MAX, so that the rank
// (N - 1) / 2 of the padded set is the rank (n - 1) / 2 of the real keys.  Neither sentinel is the key of a finite float.
// n == 0 is the caller's to test.
template <int R>
__device__ __forceinline__ int mf_window_registers(const int2* base, int cols, int* mu, int* mv)
{
    constexpr int S = 2 * R + 1, N = S * S;
    int ku[N], kv[N];
    int n = 0;
#pragma unroll
    for (int dy = 0; dy < S; dy++)
#pragma unroll
        for (int dx = 0; dx < S; dx++) {
            const int2 k = base[dy * cols + dx];
            ku[dy * S + dx] = k.x;
            kv[dy * S + dx] = k.y;
            n += k.x != MF_MARK ? 1 : 0;
        }
    if (n != N) {
        const int low = (N - 1) / 2 - (n - 1) / 2;
        int seen = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const bool missing = ku[i] == MF_MARK;
            const int s = seen < low ? INT_MIN : INT_MAX;
            ku[i] = missing ? s : ku[i];
            kv[i] = missing ? s : kv[i];
            seen += missing ? 1 : 0;
        }
    }
    *mu = mf_select<N>(ku);
    *mv = mf_select<N>(kv);
    return n;
}

// Generic path: n, and for n > 0 the keys of rank (n - 1) / 2 of both components, by bisection between the window's
// smallest and largest key.
__device__ __forceinline__ int mf_window_bisect(const int2* base, int cols, int r, int* mu, int* mv)
{
    const int S = 2 * r + 1;
    int n = 0, lou = INT_MAX, lov = INT_MAX, hiu = INT_MIN, hiv = INT_MIN;
    for (int dy = 0; dy < S; dy++) {
        const int2* line = base + dy * cols;
        for (int dx = 0; dx < S; dx++) {
            const int2 k = line[dx];
            const bool part = k.x != MF_MARK;
            n += part ? 1 : 0;
            lou = mf_min(lou, k.x);
            lov = mf_min(lov, k.y);
            hiu = mf_max(hiu, part ? k.x : INT_MIN);
            hiv = mf_max(hiv, part ? k.y : INT_MIN);
        }
    }
    if (n == 0) return 0;
    const int need = (n - 1) / 2 + 1;
    // the answer is in [lo, hi], and at least `need` keys are <= hi: both hold from here to the end
    while (lou < hiu || lov < hiv) {
        const int pu = lou + (int)(((unsigned)hiu - (unsigned)lou) >> 1);
        const int pv = lov + (int)(((unsigned)hiv - (unsigned)lov) >> 1);
        int cu = 0, cv = 0;
        for (int dy = 0; dy < S; dy++) {
            const int2* line = base + dy * cols;
            for (int dx = 0; dx < S; dx++) {
                const int2 k = line[dx];
                cu += k.x <= pu ? 1 : 0;
                cv += k.y <= pv ? 1 : 0;
            }
        }
        if (cu >= need) hiu = pu;
        else lou = pu + 1;
        if (cv >= need) hiv = pv;
        else lov = pv + 1;
    }
    *mu = lou;
    *mv = lov;
    return n;
}

// R = 0: the generic kernel, radius r; R >= 1: the register kernel of radius R (r is ignored).
// counts: NULL, or {outliers, dropped, unsupported}.  out or keep may be NULL.
template <int KIND, int R>
__global__ __launch_bounds__(256) void mf_kernel(const float2* __restrict__ flow, int H, int W, MaWeight wt, int r_any, int mode,
                                                 float thresh, int nbx, float2* __restrict__ out,
                                                 unsigned char* __restrict__ keep, unsigned long long* __restrict__ counts)
{
    constexpr int RM = R ? R : MA_MEDIAN_MAX_RADIUS;
    __shared__ __attribute__((aligned(8))) int tile_words[(MF_TH + 2 * RM) * (MF_TW + 2 * RM) * 2];
    int2* tile = reinterpret_cast<int2*>(tile_words);          // [rows][cols], (key of u, key of v)
    const int r = R ? R : r_any;
    const int cols = MF_TW + 2 * r, rows = MF_TH + 2 * r;
    const int x0 = (int)(blockIdx.x % nbx) * MF_TW, y0 = (int)(blockIdx.x / nbx) * MF_TH;
    for (int t = threadIdx.x; t < rows * cols; t += 256) {
        const int j = t / cols, c = t - j * cols;
        const int y = y0 - r + j, x = x0 - r + c;
        int2 k = make_int2(MF_MARK, MF_MARK);
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t i = (size_t)y * W + x;
            const float2 f = flow[i];
            const float wgt = d_weight_at<KIND>(wt, i, x, y);
            if (d_weight_counts(wgt) && d_finite(f.x) && d_finite(f.y)) k = make_int2(mf_key(f.x), mf_key(f.y));
        }
        tile[t] = k;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x = x0 + lane;
    unsigned int outliers = 0, dropped = 0, unsupported = 0;
#pragma unroll 1
    for (int q = 0; q < MF_ROWS; q++) {
        const int ly = wv * MF_ROWS + q, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int2* base = tile + ly * cols + lane;
        int mu = 0, mv = 0, n;
        if constexpr (R != 0) n = mf_window_registers<R>(base, cols, &mu, &mv);
        else n = mf_window_bisect(base, cols, r, &mu, &mv);
        float2 m = make_float2(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000));
        if (n > 0) m = make_float2(mf_value(mu), mf_value(mv));
        else unsupported++;
        const int2 kc = base[r * cols + r];
        float2 o = m;
        bool bad = true;
        if (kc.x != MF_MARK) {          // the pixel participates, so n > 0 and m is finite
            const float2 f = make_float2(mf_value(kc.x), mf_value(kc.y));
            const float d = fmaxf(fabsf(f.x - m.x), fabsf(f.y - m.y));
            bad = d > thresh;
            outliers += bad ? 1u : 0u;
            if (mode == MA_MEDIAN_OUTLIERS && !bad) o = f;
        } else {
            dropped++;
        }
        const size_t i = (size_t)y * W + x;
        if (out) out[i] = o;
        if (keep) keep[i] = bad ? 0 : 1;
    }
    if (counts) d_wave_tally(counts, {outliers, dropped, unsupported});     // wave-uniform
}

template <int KIND, int R>
static void mf_launch_one(ma_ctx* ctx, unsigned grid, const float* flow, int H, int W, const MaWeight& wt, int r, int mode,
                          float thresh, int nbx, float* out, unsigned char* keep, unsigned long long* counts)
{
    hipLaunchKernelGGL((mf_kernel<KIND, R>), dim3(grid), dim3(256), 0, ctx->stream, (const float2*)flow, H, W, wt, r, mode, thresh,
                       nbx, (float2*)out, keep, counts);
}

template <int KIND>
static void mf_launch(ma_ctx* ctx, bool generic, unsigned grid, const float* flow, int H, int W, const MaWeight& wt, int r,
                      int mode, float thresh, int nbx, float* out, unsigned char* keep, unsigned long long* counts)
{
    static_assert(MF_REG_MAX_RADIUS == 3, "one case per radius of the register path");
    if (!generic && r == 1) mf_launch_one<KIND, 1>(ctx, grid, flow, H, W, wt, r, mode, thresh, nbx, out, keep, counts);
    else if (!generic && r == 2) mf_launch_one<KIND, 2>(ctx, grid, flow, H, W, wt, r, mode, thresh, nbx, out, keep, counts);
    else if (!generic && r == 3) mf_launch_one<KIND, 3>(ctx, grid, flow, H, W, wt, r, mode, thresh, nbx, out, keep, counts);
    else mf_launch_one<KIND, 0>(ctx, grid, flow, H, W, wt, r, mode, thresh, nbx, out, keep, counts);
}

} // namespace

extern "C" int ma_median_flow(ma_ctx* ctx, const float* flow, int H, int W, int r, const void* weight, int weight_kind,
                              int cell_h, int cell_w, int mode, float thresh, int flags, float* out, unsigned char* keep,
                              long long* counts_host)
{
    MA_REQUIRE(ctx && flow && (out || keep), "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_REQUIRE(out != flow, "out and flow must be distinct arrays: a median reads its neighbours");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= MF_SIDE_MAX && W <= MF_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(r >= 1 && r <= MA_MEDIAN_MAX_RADIUS, "r must be in [1, 7]");
    MA_TRY(ma_weight_check(weight, weight_kind, true, {out, keep}, cell_h, cell_w));
    MA_REQUIRE(mode == MA_MEDIAN_ALL || mode == MA_MEDIAN_OUTLIERS, "unknown mode");
    MA_REQUIRE(thresh >= 0.f, "thresh must not be NaN or negative");
    MA_REQUIRE((flags & ~MA_MEDIAN_GENERIC) == 0, "unknown flags");
    const long long nbx = (W + MF_TW - 1) / MF_TW, nby = (H + MF_TH - 1) / MF_TH;
    MA_REQUIRE(nbx * nby <= 0x7fffffffLL, "flow too large: more than 2^31 - 1 tiles of 32 x 64 pixels");
    MA_HIP(hipSetDevice(ctx->device));
    unsigned long long* counts;
    MA_TRY(ma_call_counts(ctx, counts_host != nullptr, 3, &counts));
    const MaWeight wt = ma_weight_map(weight, weight_kind, W, cell_h, cell_w);
    const bool generic = (flags & MA_MEDIAN_GENERIC) != 0 || r > MF_REG_MAX_RADIUS;
    const unsigned grid = (unsigned)(nbx * nby);
    ma_weight_dispatch(weight_kind, [&](auto kind) {
        mf_launch<kind()>(ctx, generic, grid, flow, H, W, wt, r, mode, thresh, (int)nbx, out, keep, counts);
    });
    MA_HIP(hipGetLastError());
    if (counts_host) MA_TRY(ma_read_call_counts(ctx, counts, 3, counts_host));
    return MA_OK;
}
