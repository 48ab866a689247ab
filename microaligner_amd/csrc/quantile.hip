// Robust intensity normalisation (include/microaligner_quantile.h): exact order statistics of a u8 / u16 / f32 image by a
// multi-rank most-significant-digit radix select, and the scaling of an image to u8 between two given values.
//
// One pass over the image per digit (8 | 8 + 8 | 11 + 11 + 10 bits).  A pass histograms the digit of every pixel whose
// higher digits are the prefix of one of the ranks; ranks of one prefix share a histogram ("group", at most 8 of at most
// 2048 bins).  Between two passes a one-block kernel scans the histograms, fixes every rank's digit and the rank left
// inside it, and regroups the ranks; prefixes never leave the device, one synchronisation at the end brings the keys and
// the counts back.
//
// Microscopy images are mostly background: neighbouring pixels, and with them all 64 lanes of a wave, fall into one bin.
// A lane therefore reads 16 bytes of consecutive pixels and carries a run (bin, count) in registers -- through the 16
// bytes and on into its next 16 -- and only issues an LDS atomic when the bin changes: a constant background costs one
// atomic per lane and block, not one per pixel.  Block histograms live in 32-bit LDS counters (a block handles fewer than
// 2^32 pixels) and are flushed to the 64-bit global histogram with integer atomics, non-zero bins only.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "ma_internal.h"
#include "../../include/microaligner_quantile.h"

namespace {

constexpr int Q_MAXB = 2048;                  // bins of the widest digit
constexpr int Q_T = 512;                      // threads of a histogram block
constexpr int Q_SCAN_T = 256;                 // threads of the scan block
constexpr int Q_MAX_ITERS = 1 << 18;          // 16-byte reads (or single pixels) of one thread: 2^18 * 16 * 512 = 2^31 pixels a block
constexpr unsigned Q_NO_PREFIX = 0xffffffffu; // prefix of an unused group: prefixes have at most 22 bits

struct QState {
    unsigned long long excluded[2];           // nonfinite, zeros
    long long pop;
    long long rank[MA_Q_MAX_RANKS];           // the rank left inside the prefix
    unsigned prefix[MA_Q_MAX_RANKS];          // the digits fixed so far; the key after the last scan
    int group[MA_Q_MAX_RANKS];                // histogram of the rank in the coming pass
    unsigned gprefix[MA_Q_MAX_RANKS];         // prefix of every group, Q_NO_PREFIX for the unused ones
    int ngroups, pad;
};
struct QRanks { double q[MA_Q_MAX_RANKS]; int nq; };

struct QRun { int slot; unsigned cnt; };
__device__ __forceinline__ void q_run_add(QRun& r, int slot, unsigned* lds)
{
    if (slot == r.slot) { r.cnt++; return; }
    if (r.cnt) atomicAdd(&lds[r.slot], r.cnt);
    r.slot = slot; r.cnt = 1;
}

// raw: the zero-extended bits of one pixel
// NG: the groups a pass can have (1, 2, 4 or 8 >= the ranks of the call): the prefix compares of a pixel
template <typename T, bool FIRST, int NG>
__device__ __forceinline__ void q_element(unsigned raw, bool ignore_zeros, int shift, int bits, const unsigned (&gp)[NG],
                                          QRun& run, unsigned* lds, unsigned& n_nonfinite, unsigned& n_zero)
{
    unsigned key;
    if constexpr (sizeof(T) == 4) {
        if ((raw & 0x7f800000u) == 0x7f800000u) { if (FIRST) n_nonfinite++; return; }
        const unsigned b = raw == 0x80000000u ? 0u : raw;     // v + 0.0f of a finite v: -0.0 -> +0.0, nothing else changes
        if (ignore_zeros && b == 0) { if (FIRST) n_zero++; return; }
        key = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    } else {
        if (ignore_zeros && raw == 0) { if (FIRST) n_zero++; return; }
        key = raw;
    }
    const unsigned digit = (key >> shift) & ((1u << bits) - 1u);
    if constexpr (FIRST) {
        q_run_add(run, (int)digit, lds);
    } else {
        const unsigned hi = key >> (shift + bits);             // shift + bits <= 22 behind the first pass
        int g = -1;
#pragma unroll
        for (int i = 0; i < NG; i++) if (hi == gp[i]) g = i;
        if (g >= 0) q_run_add(run, (g << bits) + (int)digit, lds);
    }
}

// One digit of every pixel.  nvec: whole 16-byte groups read as vectors (0 when img is not 16-byte aligned); the pixels
// behind them are read one by one.  LDS: [ngmax << bits] counters, then the two counts of the pixels left out.
template <typename T, bool FIRST, int NG>
__global__ __launch_bounds__(Q_T) void quant_hist(const T* __restrict__ img, size_t n, size_t nvec, int ignore_zeros, int shift,
                                                  int bits, int ngmax, QState* st, unsigned long long* __restrict__ hist)
{
    extern __shared__ unsigned q_lds[];
    const int nslots = (FIRST ? 1 : ngmax) << bits;
    for (int i = threadIdx.x; i < nslots + 2; i += Q_T) q_lds[i] = 0;
    unsigned gp[NG];
#pragma unroll
    for (int i = 0; i < NG; i++) gp[i] = FIRST ? Q_NO_PREFIX : st->gprefix[i];
    __syncthreads();

    constexpr int EPV = 16 / (int)sizeof(T);
    const bool iz = ignore_zeros != 0;
    QRun run = {0, 0u};
    unsigned n_nonfinite = 0, n_zero = 0;
    const size_t stride = (size_t)gridDim.x * Q_T;
    size_t t = (size_t)blockIdx.x * Q_T + threadIdx.x;
    if (t < nvec) {
        const uint4* __restrict__ v4 = reinterpret_cast<const uint4*>(img);
        uint4 cur = v4[t];
        for (;;) {
            const size_t tn = t + stride;
            const bool more = tn < nvec;
            uint4 nxt = cur;
            if (more) nxt = v4[tn];                             // in flight while the current 16 bytes are counted
            const unsigned w[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
            for (int e = 0; e < EPV; e++) {
                unsigned raw;
                if constexpr (sizeof(T) == 1) raw = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
                else if constexpr (sizeof(T) == 2) raw = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
                else raw = w[e];
                q_element<T, FIRST, NG>(raw, iz, shift, bits, gp, run, q_lds, n_nonfinite, n_zero);
            }
            if (!more) break;
            cur = nxt;
            t = tn;
        }
    }
    for (size_t i = nvec * EPV + (size_t)blockIdx.x * Q_T + threadIdx.x; i < n; i += stride) {
        unsigned raw;
        if constexpr (sizeof(T) == 4) raw = __float_as_uint(img[i]);
        else raw = (unsigned)img[i];
        q_element<T, FIRST, NG>(raw, iz, shift, bits, gp, run, q_lds, n_nonfinite, n_zero);
    }
    if (run.cnt) atomicAdd(&q_lds[run.slot], run.cnt);
    if (FIRST) {
        if (n_nonfinite) atomicAdd(&q_lds[nslots], n_nonfinite);
        if (n_zero) atomicAdd(&q_lds[nslots + 1], n_zero);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nslots; i += Q_T) {
        const unsigned c = q_lds[i];
        if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
    if (FIRST && threadIdx.x < 2) {
        const unsigned c = q_lds[nslots + threadIdx.x];
        if (c) atomicAdd(&st->excluded[threadIdx.x], (unsigned long long)c);
    }
}

// Exclusive prefix sum over the Q_SCAN_T per-thread values of a block -> this thread's offset.  wsum: 4 LDS words.
__device__ __forceinline__ unsigned long long q_block_exscan(unsigned long long v, unsigned long long* wsum)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    __syncthreads();                       // wsum of the previous call has been read
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned long long base = 0;
    for (int k = 0; k < wv; k++) base += wsum[k];
    return base + inc - v;
}

// After pass `pass` (its histograms: hist[group][1 << bits]): the digit of every rank and the rank left inside it, then
// the groups of the coming pass.  One block of Q_SCAN_T threads.
__global__ __launch_bounds__(Q_SCAN_T) void quant_scan(QState* st, const unsigned long long* __restrict__ hist, int bits,
                                                       int pass, QRanks rk, unsigned long long n)
{
    __shared__ unsigned long long cum[Q_MAXB];
    __shared__ unsigned long long wsum[Q_SCAN_T / 64];
    __shared__ unsigned s_prefix[MA_Q_MAX_RANKS];
    const int B = 1 << bits, per = B / Q_SCAN_T;            // 1, 4 or 8 bins a thread
    const int j = threadIdx.x;
    const int nq = rk.nq;
    long long rank = 0, pop;
    unsigned prefix = 0;
    int group = 0, ngroups;
    if (pass == 0) {
        pop = (long long)(n - st->excluded[0] - st->excluded[1]);
        ngroups = pop > 0 ? 1 : 0;
        if (j < nq && pop > 0) rank = (long long)floor(rk.q[j] * (double)(pop - 1));
    } else {
        pop = st->pop;
        ngroups = st->ngroups;
        if (j < nq) { rank = st->rank[j]; prefix = st->prefix[j]; group = st->group[j]; }
    }
    for (int g = 0; g < ngroups; g++) {
        unsigned long long c[8], s = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            c[i] = i < per ? hist[((size_t)g << bits) + (size_t)j * per + i] : 0ull;
            s += c[i];
        }
        unsigned long long at = q_block_exscan(s, wsum);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (i < per) cum[j * per + i] = at;
            at += c[i];
        }
        __syncthreads();
        if (j < nq && group == g) {
            // the largest d with cum[d] <= rank: its bin is not empty and holds the rank
            int lo = 0, hi = B - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (cum[mid] <= (unsigned long long)rank) lo = mid; else hi = mid - 1;
            }
            prefix = (prefix << bits) | (unsigned)lo;
            rank -= (long long)cum[lo];
        }
        __syncthreads();
    }
    if (j < nq) s_prefix[j] = prefix;
    __syncthreads();
    if (j < nq) {
        // ranks of one prefix share the histogram of the first of them; groups are numbered in the order of their first rank
        int first = j, ng = 0;
        for (int i = j - 1; i >= 0; i--) if (s_prefix[i] == prefix) first = i;
        for (int i = 0; i < first; i++) {
            bool lead = true;
            for (int k = 0; k < i; k++) if (s_prefix[k] == s_prefix[i]) lead = false;
            ng += lead;
        }
        st->rank[j] = rank;
        st->prefix[j] = prefix;
        st->group[j] = ng;
        if (first == j && pop > 0) st->gprefix[ng] = prefix;
    }
    if (j == 0) {
        int ng = 0;
        for (int i = 0; i < nq; i++) {
            bool lead = true;
            for (int k = 0; k < i; k++) if (s_prefix[k] == s_prefix[i]) lead = false;
            ng += lead;
        }
        if (pop <= 0) ng = 0;
        st->pop = pop;
        st->ngroups = ng;
        for (int i = ng; i < MA_Q_MAX_RANKS; i++) st->gprefix[i] = Q_NO_PREFIX;
    }
}

// dst = u8(round_half_even(clamp(src * a + b, 0, 255))), a multiply and then an add.  Groups of four pixels, one packed
// 4-byte store; a scalar tail, and the scalar form throughout when a pointer is not aligned.
template <typename T>
__global__ __launch_bounds__(256) void range_to_u8(const T* __restrict__ src, size_t n, float a, float b, uint8_t* __restrict__ dst)
{
    auto cvt = [&](float x) -> unsigned {
        float v = __fadd_rn(__fmul_rn(x, a), b);
        v = fminf(fmaxf(v, 0.f), 255.f);          // a NaN becomes 0
        return (unsigned)d_clamp(d_cvround(v), 0, 255);
    };
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const bool vec = (((size_t)src & (4 * sizeof(T) - 1)) | ((size_t)dst & 3)) == 0;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = tid; i < n4; i += stride) {
        float x0, x1, x2, x3;
        if constexpr (sizeof(T) == 4) {
            const float4 q = reinterpret_cast<const float4*>(src)[i];
            x0 = q.x; x1 = q.y; x2 = q.z; x3 = q.w;
        } else if constexpr (sizeof(T) == 2) {
            const uint2 q = reinterpret_cast<const uint2*>(src)[i];
            x0 = (float)(q.x & 0xffffu); x1 = (float)(q.x >> 16); x2 = (float)(q.y & 0xffffu); x3 = (float)(q.y >> 16);
        } else {
            const unsigned q = reinterpret_cast<const unsigned*>(src)[i];
            x0 = (float)(q & 0xffu); x1 = (float)((q >> 8) & 0xffu); x2 = (float)((q >> 16) & 0xffu); x3 = (float)(q >> 24);
        }
        __builtin_nontemporal_store(cvt(x0) | (cvt(x1) << 8) | (cvt(x2) << 16) | (cvt(x3) << 24), &reinterpret_cast<unsigned*>(dst)[i]);
    }
    for (size_t i = n4 * 4 + tid; i < n; i += stride) dst[i] = (uint8_t)cvt((float)src[i]);
}

// digits of the key of a dtype, most significant first
int q_digits(int dtype, int bits[3])
{
    if (dtype == MA_U8) { bits[0] = 8; return 1; }
    if (dtype == MA_U16) { bits[0] = 8; bits[1] = 8; return 2; }
    bits[0] = 11; bits[1] = 11; bits[2] = 10;
    return 3;
}

template <typename T>
int q_launch_hist(ma_ctx* ctx, const void* img, size_t n, int flags, int pass, int shift, int bits, int nq, QState* st,
                  unsigned long long* hist)
{
    constexpr size_t EPV = 16 / sizeof(T);
    const size_t nvec = ((size_t)img & 15) == 0 ? n / EPV : 0;
    const size_t units = nvec ? nvec : n;                        // the longer of the two loops of a thread
    size_t grid = (units + Q_T - 1) / Q_T;
    if (grid > 2048) grid = 2048;
    const size_t need = (units + (size_t)Q_T * Q_MAX_ITERS - 1) / ((size_t)Q_T * Q_MAX_ITERS);
    if (grid < need) grid = need;                                // 32-bit LDS counters: bound the pixels of a block
    const int iz = (flags & MA_Q_IGNORE_ZEROS) != 0;
    const size_t lds = ((size_t)((pass == 0 ? 1 : nq) << bits) + 2) * sizeof(unsigned);
#define MA_Q_HIST(FIRST, NG)                                                                                                 \
    do {                                                                                                                     \
        if (lds > 64 * 1024)                                                                                                 \
            MA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(quant_hist<T, FIRST, NG>),                              \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                               \
        hipLaunchKernelGGL((quant_hist<T, FIRST, NG>), dim3((unsigned)grid), dim3(Q_T), lds, ctx->stream, (const T*)img, n,  \
                           nvec, iz, shift, bits, nq, st, hist);                                                             \
    } while (0)
    if (pass == 0) MA_Q_HIST(true, 1);
    else if (nq <= 1) MA_Q_HIST(false, 1);
    else if (nq <= 2) MA_Q_HIST(false, 2);
    else if (nq <= 4) MA_Q_HIST(false, 4);
    else MA_Q_HIST(false, 8);
#undef MA_Q_HIST
    MA_HIP(hipGetLastError());
    return MA_OK;
}

int grid_for(size_t n) { size_t b = (n + 256 * 4 - 1) / (256 * 4); return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }

} // namespace

extern "C" {

int ma_image_quantiles(ma_ctx* ctx, const void* img, int dtype, size_t n, int flags, const double* q, int nq,
                       double* values, long long counts[3])
{
    MA_REQUIRE(ctx && img && q && values && counts, "NULL argument");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "dtype must be u8/u16/f32");
    MA_REQUIRE(n > 0, "empty array");
    MA_REQUIRE(n <= (size_t)MA_Q_MAX_PIXELS, "an image must hold at most 2^40 pixels");
    MA_REQUIRE((flags & ~MA_Q_IGNORE_ZEROS) == 0, "unknown quantile flag");
    MA_REQUIRE(nq >= 1 && nq <= MA_Q_MAX_RANKS, "1 to 8 quantiles a call");
    QRanks rk;
    rk.nq = nq;
    for (int j = 0; j < MA_Q_MAX_RANKS; j++) rk.q[j] = 0.0;
    for (int j = 0; j < nq; j++) {
        MA_REQUIRE(q[j] >= 0.0 && q[j] <= 1.0, "a quantile must lie in [0, 1]");   // false for a NaN
        rk.q[j] = q[j];
    }
    MA_HIP(hipSetDevice(ctx->device));
    int bits[3];
    const int npass = q_digits(dtype, bits);
    const size_t st_bytes = ma_align_up(sizeof(QState), 256);
    const size_t hist_bytes = (size_t)MA_Q_MAX_RANKS * Q_MAXB * sizeof(unsigned long long);
    MA_TRY(ma_ws_reserve(ctx, st_bytes + npass * hist_bytes));
    MA_TRY(ma_pinned_reserve(ctx, sizeof(QState)));
    QState* st = (QState*)ctx->ws;
    MA_HIP(hipMemsetAsync(ctx->ws, 0, st_bytes + npass * hist_bytes, ctx->stream));
    {
        MaProfScope ps(ctx, MA_K_OTHER, (double)n * npass);
        int shift = dtype == MA_U8 ? 8 : (dtype == MA_U16 ? 16 : 32);
        for (int p = 0; p < npass; p++) {
            shift -= bits[p];
            unsigned long long* hist = (unsigned long long*)((char*)ctx->ws + st_bytes + p * hist_bytes);
            if (dtype == MA_U8) MA_TRY(q_launch_hist<uint8_t>(ctx, img, n, flags, p, shift, bits[p], nq, st, hist));
            else if (dtype == MA_U16) MA_TRY(q_launch_hist<uint16_t>(ctx, img, n, flags, p, shift, bits[p], nq, st, hist));
            else MA_TRY(q_launch_hist<float>(ctx, img, n, flags, p, shift, bits[p], nq, st, hist));
            hipLaunchKernelGGL(quant_scan, dim3(1), dim3(Q_SCAN_T), 0, ctx->stream, st, hist, bits[p], p, rk, (unsigned long long)n);
            MA_HIP(hipGetLastError());
        }
    }
    MA_HIP(hipMemcpyAsync(ctx->pinned, st, sizeof(QState), hipMemcpyDeviceToHost, ctx->stream));
    MA_HIP(hipStreamSynchronize(ctx->stream));
    const QState* h = (const QState*)ctx->pinned;
    counts[0] = h->pop;
    counts[1] = (long long)h->excluded[0];
    counts[2] = (long long)h->excluded[1];
    for (int j = 0; j < nq; j++) {
        if (h->pop <= 0) { values[j] = NAN; continue; }
        const unsigned key = h->prefix[j];
        if (dtype == MA_F32) {
            const unsigned b = key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu);
            float f;
            memcpy(&f, &b, sizeof f);
            values[j] = (double)f;
        } else {
            values[j] = (double)key;
        }
    }
    return MA_OK;
}

int ma_normalize_range_u8(ma_ctx* ctx, const void* src, int dtype, size_t n, double lo, double hi, uint8_t* dst)
{
    MA_REQUIRE(ctx && src && dst, "NULL argument");
    MA_REQUIRE(dtype == MA_U8 || dtype == MA_U16 || dtype == MA_F32, "dtype must be u8/u16/f32");
    MA_REQUIRE(n > 0, "empty array");
    MA_REQUIRE(std::isfinite(lo) && std::isfinite(hi), "lo and hi must be finite");
    MA_HIP(hipSetDevice(ctx->device));
    const double d = hi - lo;
    const double scale = 255. * (d > DBL_EPSILON ? 1. / d : 0);
    const double shift = 0. - lo * scale;
    MaProfScope ps(ctx, MA_K_OTHER, (double)n);
    dim3 grid(grid_for(n)), block(256);
    if (dtype == MA_U8) hipLaunchKernelGGL((range_to_u8<uint8_t>), grid, block, 0, ctx->stream, (const uint8_t*)src, n, (float)scale, (float)shift, dst);
    else if (dtype == MA_U16) hipLaunchKernelGGL((range_to_u8<uint16_t>), grid, block, 0, ctx->stream, (const uint16_t*)src, n, (float)scale, (float)shift, dst);
    else hipLaunchKernelGGL((range_to_u8<float>), grid, block, 0, ctx->stream, (const float*)src, n, (float)scale, (float)shift, dst);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

} // extern "C"
