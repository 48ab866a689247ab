// Flat grey morphology: the running minimum and maximum of an image over a rectangle, and opening, closing and the two
// top-hats built from them (include/microaligner_morphology.h).  Off the measured path: nothing in register() or warp() calls
// it.
//
// One kernel, mo_pass_kernel, is every launch of a call: it filters the lines of an [nlines][len] array along len and writes
// the result TRANSPOSED, [len][nlines].  An erosion or a dilation is that pass over the rows of the image (into a workspace
// plane, (W, H)) and then over the rows of that plane, which are the image's columns (into a row-major plane or dst).  The
// layout is that of window_fir.h -- lines on the lanes, an odd LDS pitch, coalesced staging, transposed output -- with a
// narrower and longer tile, because a radius of 255 needs a halo of 510:
//   - tile: MO_LINES = 32 lines x MO_S = 256 outputs, 512 threads; a thread is (line = tid & 31, seg = tid >> 5) and makes
//     the MO_B = 16 consecutive outputs of its segment.  A half-wave holds 32 lines at one offset: 32 banks, no conflict;
//   - staging: a wave reads a line's span (outputs + a halo of r rounded up to 16 on either side) as int32 keys into LDS
//     [32][pitch], in whole 4-byte words aligned by the line's own address, single elements at the ends of the line.
//     Outside the image, and for a float32 NaN, the key is the sentinel: the identity of the operation;
//   - filter, r <= 7: the 2 r + 1 taps of an output straight from the thread's 16 + 2 r staged keys, held in registers;
//   - filter, r >= 8, with r = 16 k + m: the windows of a thread's 16 outputs all hold [c0 + 16 - r, c0 + r - 1] (c0 the
//     thread's first output).  That middle is the minima of the 2 k - 1 aligned blocks of 16 keys inside it, which the
//     block's threads reduce once into LDS, and m single keys at either end (k = 0: its 2 r - 16 keys).  Left of it, output q
//     adds the suffix minimum from q of the 16 keys [c0 - r, c0 - r + 15]; right of it the prefix minimum up to q of the
//     16 keys [c0 + r, c0 + r + 15].  Per 16 outputs: 32 + 2 m + 2 k - 1 LDS reads and 62 + 2 m + 2 k - 1 operations, and
//     (k + 7) / 8 reads and operations per output for the block minima: 7.6 + 2.75 operations per output at r = 255
//     where one per tap would be 511;
//   - output: lane = line, and a line of the input is a column of the output, so a half-wave stores 32 consecutive
//     elements.  The last launch of a hat reads the pixel's own x there and stores the difference.
// LDS is sized by r at launch (mo_lds): 36 KiB at r <= 15, 39 KiB at r = 16, 51 KiB at r = 64, 64 KiB at r = 97 .. 112,
// 102 KiB at r = 255 (one block per CU; the three dtypes then take 1 : 1.7 : 2.6 of a launch's time on the same
// instructions: the halo's loads under that occupancy, not the filter).
#include "../../include/microaligner_morphology.h"
#include "ma_internal.h"

#include <climits>

namespace {

constexpr int MO_SIDE_MAX = 1 << 24;
constexpr int MO_LINES = 32, MO_SEGS = 16, MO_B = 16;   // lines per tile, segments per line, outputs per segment and block size
constexpr int MO_S = MO_SEGS * MO_B;                    // outputs per line and tile
constexpr int MO_THREADS = MO_LINES * MO_SEGS;
constexpr int MO_DIRECT_MAX = 7;                        // radii up to which an output reads its taps
static_assert(MO_THREADS == 512 && MO_B == 16 && 2 * MO_DIRECT_MAX < MO_B, "the kernel is written for these");

enum { MO_PLAIN = 0, MO_TOPHAT = 1, MO_BLACKHAT = 2 };   // the epilogue of a pass

// the halo of a staged line either side of its outputs: r rounded up to whole blocks, at least one block
inline __host__ __device__ int mo_halo(int r) { return r <= MO_B ? MO_B : (r + MO_B - 1) & ~(MO_B - 1); }

template <bool MAX>
__device__ __forceinline__ int mo_op(int a, int b)
{
    return MAX ? (a > b ? a : b) : (a < b ? a : b);
}

// the identity of the operation: the key of a pixel outside the image and of a NaN
template <bool MAX>
constexpr int mo_sentinel() { return MAX ? INT_MIN : INT_MAX; }

template <bool MAX>
__device__ __forceinline__ int mo_key(unsigned char v) { return (int)v; }
template <bool MAX>
__device__ __forceinline__ int mo_key(unsigned short v) { return (int)v; }
template <bool MAX>
__device__ __forceinline__ int mo_key(float v)
{
    const int bits = __float_as_int(v);
    if ((bits & 0x7fffffff) > 0x7f800000) return mo_sentinel<MAX>();
    return bits ^ ((bits >> 31) & 0x7fffffff);
}

template <typename T, bool MAX>
__device__ __forceinline__ T mo_value(int key)
{
    if constexpr (sizeof(T) == 4) {
        if (key == mo_sentinel<MAX>()) return __int_as_float(0x7fc00000);
        return __int_as_float(key ^ ((key >> 31) & 0x7fffffff));
    } else {
        return (T)key;
    }
}

// a - b of a hat
__device__ __forceinline__ unsigned char mo_minus(unsigned char a, unsigned char b) { return (unsigned char)(a - b); }
__device__ __forceinline__ unsigned short mo_minus(unsigned short a, unsigned short b) { return (unsigned short)(a - b); }
__device__ __forceinline__ float mo_minus(float a, float b)
{
    const float d = a - b;
    return d == d ? d : __int_as_float(0x7fc00000);
}

// One line into LDS as keys.  g0: the index in src of the element that line[0] stands for, which may lie in front of the
// line; ps: that element's position on the line; positions outside [0, len) give the sentinel.  Where an element has
// fewer than 4 bytes the wave reads whole words aligned by the address itself, so every word inside the line is inside the
// array; the words that straddle an end of the line or of the span are read element by element.
template <typename T, bool MAX>
__device__ __forceinline__ void mo_stage_line(const T* src, long long g0, int ps, int len, int span, int lane, int* line)
{
    constexpr int E = 4 / (int)sizeof(T);
    constexpr int SENT = mo_sentinel<MAX>();
    if constexpr (E == 1) {
        for (int c = lane; c < span; c += 64) {
            const int p = ps + c;
            line[c] = (p >= 0 && p < len) ? mo_key<MAX>(src[g0 + c]) : SENT;
        }
    } else {
        constexpr int BITS = 8 * (int)sizeof(T);
        const int mis = (int)(((long long)((uintptr_t)src / sizeof(T)) + g0) & (E - 1));
        const int nwords = (span + mis + E - 1) / E;
        for (int i = lane; i < nwords; i += 64) {
            const int cb = i * E - mis, pb = ps + cb;
            if (cb >= 0 && cb + E <= span && pb >= 0 && pb + E <= len) {
                const unsigned word = *reinterpret_cast<const unsigned*>(src + (g0 + cb));
#pragma unroll
                for (int j = 0; j < E; j++) line[cb + j] = (int)((word >> (j * BITS)) & ((1u << BITS) - 1u));
            } else {
#pragma unroll
                for (int j = 0; j < E; j++) {
                    const int c = cb + j, p = ps + c;
                    if (c >= 0 && c < span) line[c] = (p >= 0 && p < len) ? mo_key<MAX>(src[g0 + c]) : SENT;
                }
            }
        }
    }
}

// the 16 outputs from c0 of a line at a radius R <= MO_DIRECT_MAX: every tap of every output, from registers
template <int R, bool MAX>
__device__ __forceinline__ void mo_direct(const int* line, int c0, int (&v)[MO_B])
{
    int w[MO_B + 2 * R];
#pragma unroll
    for (int j = 0; j < MO_B + 2 * R; j++) w[j] = line[c0 - R + j];
#pragma unroll
    for (int q = 0; q < MO_B; q++) {
        int a = w[q + R];
#pragma unroll
        for (int t = 1; t <= R; t++) a = mo_op<MAX>(a, mo_op<MAX>(w[q + R - t], w[q + R + t]));
        v[q] = a;
    }
}

// One pass.  src: [nlines][len]; dst and, for a hat, orig: [len][nlines].  Block: lines [l0, l0 + 32) x outputs
// [p0, p0 + 256).  dst may be orig (a hat in place): a thread reads orig[i] before it writes dst[i] and no other thread
// touches i; dst is never src.
template <typename T, bool MAX, int EPI>
__global__ __launch_bounds__(MO_THREADS) void mo_pass_kernel(const T* src, int nlines, int len, int r, int nbl, T* dst, const T* orig)
{
    extern __shared__ int lds[];   // [32][pitch] keys, then [32][bpitch] block minima
    constexpr int SENT = mo_sentinel<MAX>();
    const int tid = threadIdx.x, lane = tid & 63, line = tid & (MO_LINES - 1), seg = tid >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int halo = mo_halo(r), span = MO_S + 2 * halo, pitch = span | 1;
    const int p0 = (int)(blockIdx.x % (unsigned)nbl) * MO_S, l0 = (int)(blockIdx.x / (unsigned)nbl) * MO_LINES;
    for (int row = wv; row < MO_LINES; row += MO_THREADS / 64) {
        const int l = l0 + row;
        int* dstline = lds + row * pitch;
        if (l < nlines) {
            mo_stage_line<T, MAX>(src, (long long)l * len + (p0 - halo), p0 - halo, len, span, lane, dstline);
        } else {
            for (int c = lane; c < span; c += 64) dstline[c] = SENT;
        }
    }
    __syncthreads();
    const int k = r >> 4, m = r & (MO_B - 1);
    const int nblk = span / MO_B, bpitch = nblk | 1;
    int* bmin = lds + MO_LINES * pitch;
    const int* mine = lds + line * pitch;
    if (k >= 1) {   // block-uniform
        // the blocks that some thread's middle holds: halo / 16 + 1 - k .. halo / 16 + 15 + k - 1
        const int lo = halo / MO_B + 1 - k, hi = halo / MO_B + MO_SEGS - 2 + k;
        for (int b = lo + seg; b <= hi; b += MO_SEGS) {
            const int* blk = mine + b * MO_B;
            int a = blk[0];
#pragma unroll
            for (int j = 1; j < MO_B; j++) a = mo_op<MAX>(a, blk[j]);
            bmin[line * bpitch + b] = a;
        }
        __syncthreads();
    }
    const int c0 = halo + seg * MO_B;
    int v[MO_B];
    if (r <= MO_DIRECT_MAX) {   // block-uniform
        switch (r) {
        case 0: mo_direct<0, MAX>(mine, c0, v); break;
        case 1: mo_direct<1, MAX>(mine, c0, v); break;
        case 2: mo_direct<2, MAX>(mine, c0, v); break;
        case 3: mo_direct<3, MAX>(mine, c0, v); break;
        case 4: mo_direct<4, MAX>(mine, c0, v); break;
        case 5: mo_direct<5, MAX>(mine, c0, v); break;
        case 6: mo_direct<6, MAX>(mine, c0, v); break;
        default: mo_direct<7, MAX>(mine, c0, v); break;
        }
    } else {
        int left[MO_B], right[MO_B];
#pragma unroll
        for (int j = 0; j < MO_B; j++) {
            left[j] = mine[c0 - r + j];
            right[j] = mine[c0 + r + j];
        }
#pragma unroll
        for (int j = MO_B - 2; j >= 0; j--) left[j] = mo_op<MAX>(left[j], left[j + 1]);     // suffix: [c0 - r + j, c0 - r + 15]
#pragma unroll
        for (int j = 1; j < MO_B; j++) right[j] = mo_op<MAX>(right[j], right[j - 1]);      // prefix: [c0 + r, c0 + r + j]
        int mid = SENT;   // [c0 + 16 - r, c0 + r - 1]
        if (k == 0) {
            for (int c = c0 + MO_B - r; c < c0 + r; c++) mid = mo_op<MAX>(mid, mine[c]);
        } else {
            for (int j = 0; j < m; j++) mid = mo_op<MAX>(mid, mo_op<MAX>(mine[c0 + MO_B - r + j], mine[c0 + MO_B * k + j]));
            const int* bm = bmin + line * bpitch + c0 / MO_B;
            for (int b = 1 - k; b <= k - 1; b++) mid = mo_op<MAX>(mid, bm[b]);
        }
#pragma unroll
        for (int q = 0; q < MO_B; q++) v[q] = mo_op<MAX>(mo_op<MAX>(left[q], right[q]), mid);
    }
    const int l = l0 + line;
    if (l >= nlines) return;
#pragma unroll
    for (int q = 0; q < MO_B; q++) {
        const int p = p0 + seg * MO_B + q;
        if (p >= len) continue;
        const size_t i = (size_t)p * nlines + l;
        T out = mo_value<T, MAX>(v[q]);
        if (EPI == MO_TOPHAT) out = mo_minus(orig[i], out);
        if (EPI == MO_BLACKHAT) out = mo_minus(out, orig[i]);
        dst[i] = out;
    }
}

// bytes of dynamic LDS of a pass at radius r
inline size_t mo_lds(int r)
{
    const int span = MO_S + 2 * mo_halo(r);
    return (size_t)MO_LINES * ((span | 1) + (r >= MO_B ? (span / MO_B) | 1 : 0)) * sizeof(int);
}

// blocks of a pass over an [nlines][len] array
inline int mo_grid(int nlines, int len, unsigned* blocks, int* nbl)
{
    const long long a = (len + MO_S - 1) / MO_S, b = (nlines + MO_LINES - 1) / MO_LINES;
    // a launch holds fewer than 2^32 threads along x
    if (a * b * MO_THREADS > 0xffffffffLL) {
        ma_set_error("invalid argument: image too large");
        return MA_EINVAL;
    }
    *blocks = (unsigned)(a * b);
    *nbl = (int)a;
    return MA_OK;
}

template <typename T, bool MAX, int EPI>
static int mo_launch(ma_ctx* ctx, const T* src, int nlines, int len, int r, T* dst, const T* orig)
{
    unsigned blocks;
    int nbl;
    MA_TRY(mo_grid(nlines, len, &blocks, &nbl));
    const size_t lds = mo_lds(r);
    if (lds >= 64 * 1024)   // r >= 97: at or above what a kernel has without asking
        MA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mo_pass_kernel<T, MAX, EPI>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((mo_pass_kernel<T, MAX, EPI>), dim3(blocks), dim3(MO_THREADS), lds, ctx->stream, src, nlines, len, r, nbl,
                       dst, orig);
    return MA_OK;
}

// an erosion (max == false) or a dilation of the (H, W) image src into dst through the plane tmp, (W, H); epi: the
// epilogue of the second launch against orig
template <typename T>
static int mo_primitive(ma_ctx* ctx, bool max, const T* src, int H, int W, int ry, int rx, T* tmp, T* dst, int epi, const T* orig)
{
    if (max) {
        MA_TRY((mo_launch<T, true, MO_PLAIN>(ctx, src, H, W, rx, tmp, nullptr)));
        if (epi == MO_TOPHAT) return mo_launch<T, true, MO_TOPHAT>(ctx, tmp, W, H, ry, dst, orig);
        return mo_launch<T, true, MO_PLAIN>(ctx, tmp, W, H, ry, dst, nullptr);
    }
    MA_TRY((mo_launch<T, false, MO_PLAIN>(ctx, src, H, W, rx, tmp, nullptr)));
    if (epi == MO_BLACKHAT) return mo_launch<T, false, MO_BLACKHAT>(ctx, tmp, W, H, ry, dst, orig);
    return mo_launch<T, false, MO_PLAIN>(ctx, tmp, W, H, ry, dst, nullptr);
}

template <typename T>
static int mo_run(ma_ctx* ctx, const T* src, int H, int W, int op, int ry, int rx, T* ws, T* dst)
{
    T* tmp = ws;                          // (W, H): the row pass of either step
    T* step = ws + (size_t)H * W;         // (H, W): the first step of the four two-step ops
    switch (op) {
    case MA_MORPH_ERODE: return mo_primitive<T>(ctx, false, src, H, W, ry, rx, tmp, dst, MO_PLAIN, nullptr);
    case MA_MORPH_DILATE: return mo_primitive<T>(ctx, true, src, H, W, ry, rx, tmp, dst, MO_PLAIN, nullptr);
    case MA_MORPH_OPEN:
    case MA_MORPH_TOPHAT:
        MA_TRY(mo_primitive<T>(ctx, false, src, H, W, ry, rx, tmp, step, MO_PLAIN, nullptr));
        return mo_primitive<T>(ctx, true, step, H, W, ry, rx, tmp, dst, op == MA_MORPH_TOPHAT ? MO_TOPHAT : MO_PLAIN, src);
    default:   // MA_MORPH_CLOSE, MA_MORPH_BLACKHAT
        MA_TRY(mo_primitive<T>(ctx, true, src, H, W, ry, rx, tmp, step, MO_PLAIN, nullptr));
        return mo_primitive<T>(ctx, false, step, H, W, ry, rx, tmp, dst, op == MA_MORPH_BLACKHAT ? MO_BLACKHAT : MO_PLAIN, src);
    }
}

} // namespace

extern "C" int ma_morphology(ma_ctx* ctx, const void* src, int dtype, int H, int W, int op, int ry, int rx, void* dst)
{
    MA_REQUIRE(ctx && src && dst, "NULL argument");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "unknown dtype");
    MA_REQUIRE(op >= MA_MORPH_ERODE && op <= MA_MORPH_BLACKHAT, "unknown op");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= MO_SIDE_MAX && W <= MO_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_REQUIRE(ry >= 0 && ry <= MA_MORPH_MAX_RADIUS && rx >= 0 && rx <= MA_MORPH_MAX_RADIUS, "radii must be in [0, 255]");
    unsigned blocks;
    int nbl;
    MA_TRY(mo_grid(H, W, &blocks, &nbl));
    MA_TRY(mo_grid(W, H, &blocks, &nbl));
    const size_t elem = dtype == MA_U8 ? 1 : (dtype == MA_U16 ? 2 : 4);
    const int planes = op == MA_MORPH_ERODE || op == MA_MORPH_DILATE ? 1 : 2;
    MA_HIP(hipSetDevice(ctx->device));
    void* ws = ma_pool_alloc(ctx, (size_t)H * W * elem * planes);
    if (!ws) return MA_ENOMEM;
    int rc;
    switch (dtype) {
    case MA_U8: rc = mo_run<unsigned char>(ctx, (const unsigned char*)src, H, W, op, ry, rx, (unsigned char*)ws, (unsigned char*)dst); break;
    case MA_U16: rc = mo_run<unsigned short>(ctx, (const unsigned short*)src, H, W, op, ry, rx, (unsigned short*)ws, (unsigned short*)dst); break;
    default: rc = mo_run<float>(ctx, (const float*)src, H, W, op, ry, rx, (float*)ws, (float*)dst); break;
    }
    if (rc == MA_OK && hipGetLastError() != hipSuccess) {
        ma_set_error("a launch of ma_morphology failed");
        rc = MA_EHIP;
    }
    // stream-ordered reuse: the next call on this ctx that takes the buffer runs behind the kernels launched here
    ma_pool_free(ctx, ws);
    return rc;
}
