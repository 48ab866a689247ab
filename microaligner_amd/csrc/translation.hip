// Global translation search (include/microaligner_translation.h): the five integer moments of two u8 label images at every
// shift of a window, each over that shift's own overlap; on the host, the scores in 128-bit integers and float64, the peak
// and its refinement.  Off the measured path: nothing in register() or warp() calls it.
//
// Every moment is an integer and is summed exactly (u32 inside a block, u64 beyond), so the tables do not depend on the
// tiling, the chunking or the order of the atomics.
#include "ma_internal.h"
#include "../../include/microaligner_translation.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace {

typedef unsigned long long u64;

// ---- S_ab -------------------------------------------------------------------------------------------------------------
// The grid is blocks of shifts x chunks of the image.  A block of shifts is a rectangle of up to TR_SBX x TR_SBY shifts; a
// chunk is `tpb` tiles of TR_TH rows down one strip of TR_TW columns.  Per tile the block stages, as packed bytes in LDS,
// the tile of `a` and the tile of `b` moved by the block's first shift with a halo of the block's extent, both zero outside
// the image: a product with a pixel outside the image is zero, so the sum over the whole tile is the sum over O(d) and no
// shift needs its domain spelt out.
//
// A thread keeps the S_ab of four consecutive dx of one dy in registers for the whole chunk (where a block has fewer than
// 256 such quads, G threads share a quad, each taking every G-th row).  It walks a row four pixels at a time: the `a` word is
// the same for every lane of a row (an LDS broadcast); the dword of `b` read in the step before and one new dword give,
// through v_alignbyte_b32, the `b` words of the four shifts, and four v_dot4_u32_u8 add the products: two LDS reads for
// sixteen products.
//
// u32 bound: a step adds at most 4 * 255^2 = 260 100 to an accumulator, a thread makes at most
// tpb * ceil(TR_TH / G) * TR_KW <= 16 * 32 * 32 = 16 384 steps in a chunk, and 16 384 * 260 100 = 4 261 478 400 < 2^32.
// At the end of the chunk the sums are widened and added to the shifts' u64 in global memory: by the thread itself where it
// has its quad alone (one atomic per shift for up to 16 384 dot products of the thread), through u64 sums of the block in
// LDS where G threads share a quad (one atomic per shift and block).
constexpr int TR_NT = 256, TR_TW = 128, TR_TH = 32, TR_KW = TR_TW / 4, TR_APD = TR_KW + 1;
constexpr int TR_SBX = 32, TR_SBY = 32, TR_MAX_TPB = 16;
constexpr int TR_BR = TR_TH + TR_SBY - 1;
// dwords per staged row of b: TR_TW + TR_SBX - 1 bytes and one more dword (the walk reads one dword ahead) are 41; the
// lanes of half a wave read 8 consecutive dwords of each of 4 consecutive rows at once, and 56 = 24 (mod 32) puts those on
// 32 different banks
constexpr int TR_BPD = 56;
static_assert((TR_TW + TR_SBX - 1 + 3) / 4 + 1 <= TR_BPD, "a staged row of b must fit");
static_assert((long long)TR_MAX_TPB * TR_TH * TR_KW * 4 * 255 * 255 < (1LL << 32), "the u32 partial sums must not wrap");

struct TrWin {
    int dx0, dy0, nx, ny;       // the window as the caller gave it: the layout of the tables
    int ex0, ey0, enx, eny;     // the shifts among them with n > 0 (|dx| < w, |dy| < h): the ones any kernel touches
    int sbx, sby, nq, nbx, G;   // shifts of a block per axis, quads of dx per block row, blocks along dx, threads per quad
};

// bytes (y, x .. x + 3) of the image as one little-endian word; 0 for every byte outside the image
__device__ __forceinline__ unsigned tr_load4(const uint8_t* __restrict__ img, int h, int w, long long y, long long x)
{
    if (y < 0 || y >= h || x + 4 <= 0 || x >= w) return 0u;
    const uint8_t* p = img + (size_t)y * (size_t)w;
    if (x >= 0 && x + 4 <= w) {
        unsigned v;
        __builtin_memcpy(&v, p + x, 4);
        return v;
    }
    unsigned v = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (x + q >= 0 && x + q < w) v |= (unsigned)p[x + q] << (8 * q);
    return v;
}

__global__ __launch_bounds__(TR_NT) void tr_corr_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int h, int w,
                                                        TrWin W, int nchunk, int tpb, u64* __restrict__ mom)
{
    __shared__ unsigned A[TR_TH * TR_APD];
    __shared__ u64 Bq[(TR_BR * TR_BPD + 1) / 2];      // the tile of b; at the end, where threads share a quad, the block's sums
    unsigned* B = reinterpret_cast<unsigned*>(Bq);
    const int t = threadIdx.x;
    const int strip = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
    const int sbi = blockIdx.y % W.nbx, sbj = blockIdx.y / W.nbx;
    const int bx0 = W.ex0 + sbi * W.sbx, by0 = W.ey0 + sbj * W.sby;          // the block's first shift
    const int bnx = min(W.sbx, W.ex0 + W.enx - bx0), bny = min(W.sby, W.ey0 + W.eny - by0);   // and how many it has
    const long long tx0 = (long long)strip * TR_TW;
    const long long cy0 = (long long)chunk * tpb * TR_TH, cy1 = min(cy0 + (long long)tpb * TR_TH, (long long)h);
    // what the block reads of b, rows [cy0 + by0, cy1 + by0 + bny - 1) x columns [tx0 + bx0, tx0 + bx0 + TR_TW + bnx - 1),
    // misses the image: every product is zero
    if (cy1 + by0 + bny - 1 <= 0 || cy0 + by0 >= h || tx0 + bx0 + TR_TW + bnx - 1 <= 0 || tx0 + bx0 >= w) return;

    const int q = t % W.nq, dyl = (t / W.nq) % W.sby, grp = t / (W.nq * W.sby);
    const bool active = grp < W.G && dyl < bny && 4 * q < bnx;
    const int bpd = (TR_TW + bnx - 1 + 3) / 4 + 1;          // dwords of a row of b this block needs
    unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;

    for (long long ty0 = cy0; ty0 < cy1; ty0 += TR_TH) {
        const int th = (int)min((long long)TR_TH, cy1 - ty0);
        const int br = th + bny - 1;
        __syncthreads();     // the tile before is done with A and B
        for (int i = t; i < th * TR_KW; i += TR_NT) {
            const int y = i / TR_KW, k = i - y * TR_KW;
            A[y * TR_APD + k] = tr_load4(a, h, w, ty0 + y, tx0 + 4 * k);
        }
        for (int i = t; i < br * bpd; i += TR_NT) {
            const int r = i / bpd, c = i - r * bpd;
            B[r * TR_BPD + c] = tr_load4(b, h, w, ty0 + by0 + r, tx0 + bx0 + 4 * c);
        }
        __syncthreads();
        if (active) {
            for (int y = grp; y < th; y += W.G) {
                const unsigned* arow = A + y * TR_APD;
                const unsigned* brow = B + (y + dyl) * TR_BPD + q;
                unsigned lo = brow[0];
#pragma unroll 4
                for (int k = 0; k < TR_KW; k++) {
                    const unsigned hi = brow[k + 1], av = arow[k];
                    s0 = __builtin_amdgcn_udot4(av, lo, s0, false);
                    s1 = __builtin_amdgcn_udot4(av, __builtin_amdgcn_alignbyte(hi, lo, 1u), s1, false);
                    s2 = __builtin_amdgcn_udot4(av, __builtin_amdgcn_alignbyte(hi, lo, 2u), s2, false);
                    s3 = __builtin_amdgcn_udot4(av, __builtin_amdgcn_alignbyte(hi, lo, 3u), s3, false);
                    lo = hi;
                }
            }
        }
    }
    // the last quad of a row of shifts may reach past the block's last dx: those sums are dropped
    const int o = 4 * q;
    u64* out = mom + (size_t)(by0 - W.dy0) * (size_t)W.nx + (size_t)(bx0 - W.dx0);
    if (W.G == 1) {
        if (!active) return;
        u64* dst = out + (size_t)dyl * (size_t)W.nx + o;
        if (s0) atomicAdd(&dst[0], (u64)s0);
        if (s1 && o + 1 < bnx) atomicAdd(&dst[1], (u64)s1);
        if (s2 && o + 2 < bnx) atomicAdd(&dst[2], (u64)s2);
        if (s3 && o + 3 < bnx) atomicAdd(&dst[3], (u64)s3);
        return;
    }
    // few shifts, many threads a quad and many chunks: the threads of a quad meet in LDS first, so that a block sends one
    // atomic per shift to the few addresses every block of the grid adds to
    static_assert(sizeof(Bq) >= (size_t)TR_SBX * TR_SBY * sizeof(u64), "the block's sums must fit the tile of b");
    u64* acc = Bq;                                // [sby][sbx]
    __syncthreads();                              // the last tile is done with B
    for (int i = t; i < W.sby * W.sbx; i += TR_NT) acc[i] = 0ull;
    __syncthreads();
    if (active) {
        u64* dst = acc + dyl * W.sbx + o;
        if (s0) atomicAdd(&dst[0], (u64)s0);
        if (s1 && o + 1 < bnx) atomicAdd(&dst[1], (u64)s1);
        if (s2 && o + 2 < bnx) atomicAdd(&dst[2], (u64)s2);
        if (s3 && o + 3 < bnx) atomicAdd(&dst[3], (u64)s3);
    }
    __syncthreads();
    for (int i = t; i < bny * W.sbx; i += TR_NT) {
        const int dy = i / W.sbx, ox = i - dy * W.sbx;
        if (ox < bnx && acc[i]) atomicAdd(&out[(size_t)dy * (size_t)W.nx + ox], acc[i]);
    }
}

// ---- the four rectangle sums ------------------------------------------------------------------------------------------------
// S_a(d) is the sum of a over rows [max(0, -dy), min(h, h - dy)) x columns [max(0, -dx), min(w, w - dx)), S_b(d) the sum of b
// over the same rectangle moved by d: the column range hangs on dx alone and the row range on dy alone.  So: first the sums of
// every row over the column range of each dx (tr_rows_kernel -> [4][h][dx]), then the sums of those over the row range of each
// dy (tr_cols_kernel -> the tables).  Both are the same one-axis problem: four sequences A, AA, B, BB of length L and shifts
// e0 .. e1, |e| < L; wanted are, for every e,
//     A-kinds: the sum over j in [max(0, -e), min(L, L - e)),    B-kinds: the sum over j + e for the same j,
// which is the total less a head or a tail of |e| elements:
//     e > 0:  A = total - tail(e),   B = total - head(e);        e < 0:  A = total - head(-e),   B = total - tail(-e).
// A block of threads takes one line: the totals, the heads and tails up to the smallest |e| wanted (both by strided partial
// sums), then the wanted heads and tails as running sums over contiguous segments, one per thread, joined by a scan of the
// segment sums.  O(L + shifts) per line, whatever the shifts are.
template <int N>
__device__ __forceinline__ void tr_block_sum(u64 (&v)[N], u64* sm)
{
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; c++) sm[c * TR_NT + t] = v[c];
    __syncthreads();
    for (int s = TR_NT / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int c = 0; c < N; c++) sm[c * TR_NT + t] += sm[c * TR_NT + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < N; c++) v[c] = sm[c * TR_NT];
}

// load(j, v): v[0 .. 3] = A, AA, B, BB at position j.  store(e, kind, value), kind 0 .. 3 = A, AA, B, BB.  sm: 8 * TR_NT u64.
template <class Load, class Store>
__device__ __forceinline__ void tr_axis_sums(int L, int e0, int e1, Load load, Store store, u64* sm)
{
    const int t = threadIdx.x;
    u64 tot[4] = {0, 0, 0, 0};
    for (int j = t; j < L; j += TR_NT) {
        u64 v[4];
        load(j, v);
#pragma unroll
        for (int c = 0; c < 4; c++) tot[c] += v[c];
    }
    tr_block_sum<4>(tot, sm);
    if (t == 0 && e0 <= 0 && e1 >= 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) store(0, c, tot[c]);
    }
    // |e| of the shifts other than 0 runs over k0 .. k1
    const int k1 = max(e1, -e0);
    const int k0 = e0 > 0 ? e0 : (e1 < 0 ? -e1 : 1);
    if (k1 < k0) return;                        // the window is {0}
    // run[0 .. 3]: the head of k elements, run[4 .. 7]: the tail of k elements; first for k = k0 - 1
    u64 base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = t; j < k0 - 1; j += TR_NT) {
        u64 v[4];
        load(j, v);
#pragma unroll
        for (int c = 0; c < 4; c++) base[c] += v[c];
        load(L - 1 - j, v);
#pragma unroll
        for (int c = 0; c < 4; c++) base[4 + c] += v[c];
    }
    tr_block_sum<8>(base, sm);
    // elements k0 - 1 .. k1 - 1 in contiguous segments, one per thread
    const int cnt = k1 - k0 + 1, seg = (cnt + TR_NT - 1) / TR_NT;
    const int j0 = k0 - 1 + min(t * seg, cnt), j1 = k0 - 1 + min((t + 1) * seg, cnt);
    u64 part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = j0; j < j1; j++) {
        u64 v[4];
        load(j, v);
#pragma unroll
        for (int c = 0; c < 4; c++) part[c] += v[c];
        load(L - 1 - j, v);
#pragma unroll
        for (int c = 0; c < 4; c++) part[4 + c] += v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; c++) sm[c * TR_NT + t] = part[c];
    __syncthreads();
    if (t < 8) {                                 // exclusive scan of the segment sums, one thread per sequence
        u64 run = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) run = c == t ? base[c] : run;
        for (int i = 0; i < TR_NT; i++) {
            const u64 v = sm[t * TR_NT + i];
            sm[t * TR_NT + i] = run;
            run += v;
        }
    }
    __syncthreads();
    u64 run[8];
#pragma unroll
    for (int c = 0; c < 8; c++) run[c] = sm[c * TR_NT + t];
    for (int j = j0; j < j1; j++) {
        u64 v[4];
        load(j, v);
#pragma unroll
        for (int c = 0; c < 4; c++) run[c] += v[c];
        load(L - 1 - j, v);
#pragma unroll
        for (int c = 0; c < 4; c++) run[4 + c] += v[c];
        const int k = j + 1;
        if (k >= e0 && k <= e1) {                // e = +k: A less its tail, B less its head
            store(k, 0, tot[0] - run[4]);
            store(k, 1, tot[1] - run[5]);
            store(k, 2, tot[2] - run[2]);
            store(k, 3, tot[3] - run[3]);
        }
        if (-k >= e0 && -k <= e1) {              // e = -k: A less its head, B less its tail
            store(-k, 0, tot[0] - run[0]);
            store(-k, 1, tot[1] - run[1]);
            store(-k, 2, tot[2] - run[6]);
            store(-k, 3, tot[3] - run[7]);
        }
    }
}

// one block per image row: rows[kind][y][e - e0] for the shifts e0 .. e1 along x
__global__ __launch_bounds__(TR_NT) void tr_rows_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int h, int w,
                                                        int e0, int e1, u64* __restrict__ rows)
{
    __shared__ u64 sm[8 * TR_NT];
    const size_t y = blockIdx.x;
    const uint8_t* __restrict__ pa = a + y * (size_t)w;
    const uint8_t* __restrict__ pb = b + y * (size_t)w;
    const size_t ne = (size_t)(e1 - e0 + 1), plane = (size_t)h * ne;
    u64* __restrict__ out = rows + y * ne;
    tr_axis_sums(w, e0, e1,
                 [&](int j, u64 (&v)[4]) {
                     const u64 va = pa[j], vb = pb[j];
                     v[0] = va; v[1] = va * va; v[2] = vb; v[3] = vb * vb;
                 },
                 [&](int e, int kind, u64 val) { out[(size_t)kind * plane + (size_t)(e - e0)] = val; }, sm);
}

// one block per shift along x: the tables S_a, S_aa, S_b, S_bb at (ex0 + blockIdx.x, every dy of ey0 .. ey1)
__global__ __launch_bounds__(TR_NT) void tr_cols_kernel(const u64* __restrict__ rows, int h, int ne, int ex0, int ey0, int ey1,
                                                        TrWin W, u64* __restrict__ mom)
{
    __shared__ u64 sm[8 * TR_NT];
    const size_t plane = (size_t)h * (size_t)ne, ns = (size_t)W.nx * (size_t)W.ny;
    const u64* __restrict__ in = rows + blockIdx.x;
    u64* __restrict__ out = mom + ns + (size_t)(ex0 + (int)blockIdx.x - W.dx0);
    tr_axis_sums(h, ey0, ey1,
                 [&](int j, u64 (&v)[4]) {
#pragma unroll
                     for (int c = 0; c < 4; c++) v[c] = in[(size_t)c * plane + (size_t)j * (size_t)ne];
                 },
                 [&](int e, int kind, u64 val) { out[(size_t)kind * ns + (size_t)(e - W.dy0) * (size_t)W.nx] = val; }, sm);
}

// ---- host: checks, scores, peak ------------------------------------------------------------------------------------------
int tr_check(int h, int w, int dx0, int dx1, int dy0, int dy1, long long* nx, long long* ny)
{
    MA_REQUIRE(h >= 1 && w >= 1, "empty image");
    MA_REQUIRE((long long)h * (long long)w <= MA_TRANSLATION_MAX_PIXELS, "an image must hold at most 2^32 pixels");
    MA_REQUIRE(dx1 >= dx0 && dy1 >= dy0, "empty window");
    *nx = (long long)dx1 - dx0 + 1;
    *ny = (long long)dy1 - dy0 + 1;
    MA_REQUIRE(*nx <= MA_TRANSLATION_MAX_SHIFTS && *ny <= MA_TRANSLATION_MAX_SHIFTS && *nx * *ny <= MA_TRANSLATION_MAX_SHIFTS,
               "a window must hold at most 2^20 shifts");
    return MA_OK;
}

long long tr_count(int h, int w, long long dx, long long dy)
{
    const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    return (ax >= w || ay >= h) ? 0 : (h - ay) * (w - ax);
}

// the float64 nearest (ties to even) to an exact 128-bit integer: below 2^63 the conversion of a 64-bit integer is that; above,
// the leading 63 bits with every bit below them folded into the last one round the same way, and the scaling back is exact
double tr_to_double(__int128 v)
{
    const bool neg = v < 0;
    unsigned __int128 u = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    double d;
    if ((u >> 63) == 0) {
        d = (double)(long long)u;
    } else {
        int hb = 127;
        while (!((u >> hb) & 1)) hb--;
        const int sh = hb - 62;
        unsigned long long m = (unsigned long long)(u >> sh);
        if (u & ((((unsigned __int128)1) << sh) - 1)) m |= 1ull;
        d = std::ldexp((double)(long long)m, sh);
    }
    return neg ? -d : d;
}

double tr_score(long long n, u64 S_ab, u64 S_a, u64 S_aa, u64 S_b, u64 S_bb)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (n == 0) return nan;
    const __int128 N = n, ab = (__int128)S_ab, sa = (__int128)S_a, saa = (__int128)S_aa, sb = (__int128)S_b, sbb = (__int128)S_bb;
    const __int128 num = N * ab - sa * sb, va = N * saa - sa * sa, vb = N * sbb - sb * sb;
    if (va == 0 || vb == 0) return nan;
    return tr_to_double(num) / (std::sqrt(tr_to_double(va)) * std::sqrt(tr_to_double(vb)));
}

void tr_scores(int h, int w, int dx0, int dy0, long long nx, long long ny, const u64* mom, double* scores)
{
    const size_t ns = (size_t)(nx * ny);
    for (long long j = 0; j < ny; j++)
        for (long long i = 0; i < nx; i++) {
            const size_t s = (size_t)(j * nx + i);
            scores[s] = tr_score(tr_count(h, w, dx0 + i, dy0 + j), mom[s], mom[ns + s], mom[2 * ns + s], mom[3 * ns + s],
                                 mom[4 * ns + s]);
        }
}

inline bool tr_finite(double x) { return x - x == 0.0; }

void tr_peak(int h, int w, int dx0, int dy0, long long nx, long long ny, const double* sc, int exclude, ma_translation_result* r)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    long long best = -1, bestd2 = 0;
    for (long long j = 0; j < ny; j++)          // dy ascending, then dx ascending: among equal scores and distances the first stays
        for (long long i = 0; i < nx; i++) {
            const double v = sc[j * nx + i];
            if (!tr_finite(v)) continue;
            const long long dx = dx0 + i, dy = dy0 + j, d2 = dx * dx + dy * dy;
            if (best < 0 || v > sc[best] || (v == sc[best] && d2 < bestd2)) { best = j * nx + i; bestd2 = d2; }
        }
    r->dx = r->dy = 0;
    r->delta_x = r->delta_y = 0.0;
    r->score = r->second = nan;
    r->n = 0;
    r->at_limit = r->valid = 0;
    if (best < 0) return;
    const long long py = best / nx, px = best % nx;
    const double s0 = sc[best];
    auto refine = [&](long long pos, long long len, long long stride) {
        if (pos == 0 || pos == len - 1) return 0.0;
        const double sm = sc[best - stride], sp = sc[best + stride];
        if (!tr_finite(sm) || !tr_finite(sp)) return 0.0;
        const double den = sm - 2.0 * s0 + sp;
        if (!(den < 0.0)) return 0.0;
        const double d = 0.5 * (sm - sp) / den;
        return d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
    };
    r->dx = (int)(dx0 + px);
    r->dy = (int)(dy0 + py);
    r->delta_x = refine(px, nx, 1);
    r->delta_y = refine(py, ny, nx);
    r->score = s0;
    r->n = tr_count(h, w, r->dx, r->dy);
    r->at_limit = (px == 0 || px == nx - 1 || py == 0 || py == ny - 1) ? 1 : 0;
    r->valid = 1;
    bool any = false;
    double second = 0.0;
    for (long long j = 0; j < ny; j++)
        for (long long i = 0; i < nx; i++) {
            const long long ax = i > px ? i - px : px - i, ay = j > py ? j - py : py - j;
            if ((ax > ay ? ax : ay) <= exclude) continue;
            const double v = sc[j * nx + i];
            if (tr_finite(v) && (!any || v > second)) { second = v; any = true; }
        }
    if (any) r->second = second;
}

int tr_moments(ma_ctx* ctx, const uint8_t* ref, const uint8_t* mov, int h, int w, int dx0, int dx1, int dy0, int dy1,
               long long nx, long long ny, u64* mom)
{
    const size_t ns = (size_t)(nx * ny), mom_bytes = 5 * ns * sizeof(u64);
    TrWin W;
    W.dx0 = dx0; W.dy0 = dy0; W.nx = (int)nx; W.ny = (int)ny;
    const int ex0 = dx0 > -(w - 1) ? dx0 : -(w - 1), ex1 = dx1 < w - 1 ? dx1 : w - 1;
    const int ey0 = dy0 > -(h - 1) ? dy0 : -(h - 1), ey1 = dy1 < h - 1 ? dy1 : h - 1;
    if (ex0 > ex1 || ey0 > ey1) {                // no shift of the window has an overlap
        memset(mom, 0, mom_bytes);
        return MA_OK;
    }
    W.ex0 = ex0; W.ey0 = ey0; W.enx = ex1 - ex0 + 1; W.eny = ey1 - ey0 + 1;
    W.sbx = W.enx < TR_SBX ? (W.enx + 3) / 4 * 4 : TR_SBX;
    W.sby = W.eny < TR_SBY ? W.eny : TR_SBY;
    W.nq = W.sbx / 4;
    W.nbx = (W.enx + W.sbx - 1) / W.sbx;
    W.G = 1;
    while (W.G < TR_TH && W.nq * W.sby * W.G * 2 <= TR_NT) W.G <<= 1;
    const long long nsb = (long long)W.nbx * ((W.eny + W.sby - 1) / W.sby);
    MA_REQUIRE(nsb <= MA_GRID_Y_MAX, "too many blocks of shifts");
    // chunks: strips of TR_TW columns cut into runs of tpb tiles of TR_TH rows.  tpb trades the atomics (one per thread and
    // shift and chunk) against blocks in flight: aim at >= 4096 blocks, at most TR_MAX_TPB tiles a chunk.
    const long long nstrip = ((long long)w + TR_TW - 1) / TR_TW, ntile = ((long long)h + TR_TH - 1) / TR_TH;
    int tpb = TR_MAX_TPB;
    while (tpb > 1 && (double)nsb * (double)nstrip * (double)((ntile + tpb - 1) / tpb) < 4096.0) tpb >>= 1;
    const long long nchunk = (ntile + tpb - 1) / tpb;
    MA_REQUIRE(nstrip * nchunk <= 0x7fffffffLL, "too many chunks");

    // workspace: the tables, then the row sums of a batch of dx ([4][h][batch] u64)
    const size_t per_dx = (size_t)h * 4 * sizeof(u64);
    size_t room = ctx->ws_limit > mom_bytes ? ctx->ws_limit - mom_bytes : 0;
    if (room > ((size_t)1 << 30)) room = (size_t)1 << 30;
    long long batch = (long long)(room / per_dx);
    if (batch > W.enx) batch = W.enx;
    if (batch < 1) {
        ma_set_error("workspace limit %zu is below the %zu bytes the translation search takes", ctx->ws_limit, mom_bytes + per_dx);
        return MA_ENOMEM;
    }
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ma_ws_reserve(ctx, mom_bytes + (size_t)batch * per_dx));
    u64* d_mom = (u64*)ctx->ws;
    u64* d_rows = d_mom + 5 * ns;
    MA_HIP(hipMemsetAsync(d_mom, 0, mom_bytes, ctx->stream));
    {
        MaProfScope ps(ctx, MA_K_OTHER, (double)h * w);
        hipLaunchKernelGGL(tr_corr_kernel, dim3((unsigned)(nstrip * nchunk), (unsigned)nsb), dim3(TR_NT), 0, ctx->stream, ref, mov,
                           h, w, W, (int)nchunk, tpb, d_mom);
    }
    for (long long c0 = 0; c0 < W.enx; c0 += batch) {
        const int nb = (int)(W.enx - c0 < batch ? W.enx - c0 : batch);
        const int bx0 = ex0 + (int)c0;
        hipLaunchKernelGGL(tr_rows_kernel, dim3((unsigned)h), dim3(TR_NT), 0, ctx->stream, ref, mov, h, w, bx0, bx0 + nb - 1, d_rows);
        hipLaunchKernelGGL(tr_cols_kernel, dim3((unsigned)nb), dim3(TR_NT), 0, ctx->stream, (const u64*)d_rows, h, nb, bx0, ey0, ey1,
                           W, d_mom);
    }
    MA_HIP(hipGetLastError());
    MA_HIP(hipMemcpyAsync(mom, d_mom, mom_bytes, hipMemcpyDeviceToHost, ctx->stream));
    MA_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->profile) MA_TRY(ma_profile_flush(ctx));
    return MA_OK;
}

} // namespace

extern "C" {

int ma_translation_moments(ma_ctx* ctx, const uint8_t* ref, const uint8_t* mov, int h, int w, int dx0, int dx1, int dy0,
                           int dy1, unsigned long long* mom)
{
    MA_REQUIRE(ctx && ref && mov && mom, "NULL argument");
    long long nx, ny;
    MA_TRY(tr_check(h, w, dx0, dx1, dy0, dy1, &nx, &ny));
    return tr_moments(ctx, ref, mov, h, w, dx0, dx1, dy0, dy1, nx, ny, mom);
}

int ma_translation_scores(int h, int w, int dx0, int dx1, int dy0, int dy1, const unsigned long long* mom, double* scores)
{
    MA_REQUIRE(mom && scores, "NULL argument");
    long long nx, ny;
    MA_TRY(tr_check(h, w, dx0, dx1, dy0, dy1, &nx, &ny));
    tr_scores(h, w, dx0, dy0, nx, ny, mom, scores);
    return MA_OK;
}

int ma_translation_search(ma_ctx* ctx, const uint8_t* ref, const uint8_t* mov, int h, int w, int dx0, int dx1, int dy0,
                          int dy1, int exclude, ma_translation_result* result, double* table)
{
    MA_REQUIRE(ctx && ref && mov && result, "NULL argument");
    MA_REQUIRE(exclude >= 0, "exclude must be >= 0");
    long long nx, ny;
    MA_TRY(tr_check(h, w, dx0, dx1, dy0, dy1, &nx, &ny));
    const size_t ns = (size_t)(nx * ny);
    std::vector<u64> mom(5 * ns);
    MA_TRY(tr_moments(ctx, ref, mov, h, w, dx0, dx1, dy0, dy1, nx, ny, mom.data()));
    std::vector<double> own;
    double* sc = table;
    if (!sc) {
        own.resize(ns);
        sc = own.data();
    }
    tr_scores(h, w, dx0, dy0, nx, ny, mom.data(), sc);
    tr_peak(h, w, dx0, dy0, nx, ny, sc, exclude, result);
    return MA_OK;
}

} // extern "C"
