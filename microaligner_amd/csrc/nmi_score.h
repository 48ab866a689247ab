// The score of the mutual-information gate, stated once: the packed 16-bit LDS counters of a joint histogram, the reduction
// of a 256 x 256 joint histogram to wave partials and the f64 formula of sklearn.metrics.normalized_mutual_info_score over
// them.  nmi.hip scores the chunks of the gate with it, qc.hip the cells of a quality map: one
// body, so a cell gives the bits ma_nmi_u8 gives for the cropped cell.  Part of the measured path (build.HEADERS).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

// ---- joint histogram in LDS ---------------------------------------------------------------------------------------------
// A block holds the 256 x 256 joint histogram of its slice (or one label band of it) in LDS as 16-bit counters packed two to
// a word: a slice has at most 65 520 pixels, so no counter can reach 2^16 and a plain 32-bit LDS atomic add of
// 1 << 16 * (bin & 1) never carries into its neighbour.
constexpr int HIST_SLICE16 = 65520;

template <int NT, int WORDS>
__device__ __forceinline__ void hist16_zero(unsigned* h)
{
    for (int i = threadIdx.x; i < WORDS; i += NT) h[i] = 0;
}

__device__ __forceinline__ void hist16_add(unsigned* h, unsigned ai, unsigned bi)
{
    const unsigned bin = ai * 256u + bi;
    atomicAdd(&h[bin >> 1], 1u << ((bin & 1u) * 16u));
}

// the non-zero counters are added to the histogram in HBM (hh: the 2 * WORDS bins the LDS words stand for)
template <int NT, int WORDS>
__device__ __forceinline__ void hist16_flush(const unsigned* h, unsigned* __restrict__ hh)
{
    for (int i = threadIdx.x; i < WORDS; i += NT) {
        const unsigned c = h[i];
        if (c & 0xffffu) atomicAdd(&hh[2 * i], c & 0xffffu);
        if (c >> 16) atomicAdd(&hh[2 * i + 1], c >> 16);
    }
}

// ---- histogram -> wave partials -----------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// Four blocks of 256 threads per histogram (blockIdx.y = q): thread j of block q owns column j of the rows [64q, 64q+64),
// so the 2 x 65536 double-precision logarithms of a histogram are spread over 16 waves -- as in the single block of 1024
// threads of rounds 1 - 5, whose placement needed sixteen free wave slots on ONE CU at once and waited 380 us on average (107
// alone) for the companion stream's dog() blocks to leave (profiles/r06_kernel_stats_cfg3_companion_on.csv).  Each wave leaves
// its partial sums in `part`; nmi_final_score adds them in the order the single block used (wave 0 .. 15), so the scores keep
// their bits.
constexpr int NR_T = 256, NR_Q = 4;
// per histogram: [0..15] mutual-information partials (wave 4q + w), [16..19] / [20..23] entropy partials of a / b (the waves of
// block 0), [24..27] / [28..31] number of non-empty labels of a among the block's rows / of b (block 0 only counts them)
constexpr int NR_PART = 32;
// MOMENTS: each block also adds the exact integer moments of its rows for a Pearson correlation: sum a, sum a^2, sum ab;
// block 0 also sum b, sum b^2
constexpr int NR_MOM = 5;

// block q = blockIdx.y of NR_T threads; hh: the histogram, N: its number of pixels, out: its NR_PART partials, mom: the
// NR_MOM moments of this block (MOMENTS only)
template <bool MOMENTS>
__device__ __forceinline__ void nmi_reduce_block(const unsigned* __restrict__ hh, const double N, double* __restrict__ out,
                                                 unsigned long long* __restrict__ mom)
{
    __shared__ unsigned pa[64], pb[256];
    __shared__ int cnt[2];
    __shared__ unsigned long long sm[NR_MOM];
    const int j = threadIdx.x, q = blockIdx.y, lane = j & 63, w = j >> 6;

    if (j < 2) cnt[j] = 0;
    if (MOMENTS && j < NR_MOM) sm[j] = 0;
    // marginals (counts < 2^32 by the chunk limit): column j over ALL rows (coalesced across the wave), and -- threads 0 .. 63 --
    // row 64 q + j (64 independent 16-byte loads)
    {
        unsigned sb = 0;
#pragma unroll 16
        for (int r = 0; r < 256; r++) sb += hh[r * 256 + j];
        pb[j] = sb;
        if (j < 64) {
            const uint4* row = reinterpret_cast<const uint4*>(hh + (64 * q + j) * 256);
            unsigned sa = 0;
#pragma unroll 16
            for (int k = 0; k < 64; k++) { uint4 v = row[k]; sa += v.x + v.y + v.z + v.w; }
            pa[j] = sa;
        }
    }
    __syncthreads();
    if (j < 64 && pa[j] > 0) atomicAdd(&cnt[0], 1);
    if (q == 0 && pb[j] > 0) atomicAdd(&cnt[1], 1);
    __syncthreads();
    const double logN = log(N);
    const unsigned long long pbj = pb[j];
    double mi = 0.0;
    unsigned long long sab = 0;
    if (pbj > 0) {
#pragma unroll 8
        for (int rr = 0; rr < 64; rr++) {
            unsigned nij = hh[(64 * q + rr) * 256 + j];
            if (nij) {
                double log_nm = log((double)nij);
                double nm = (double)nij / N;
                double outer = (double)((long long)pa[rr] * (long long)pbj);
                double log_outer = -log(outer) + logN + logN;
                double term = nm * (log_nm - logN) + nm * log_outer;
                if (fabs(term) < DBL_EPSILON) term = 0.0;
                mi += term;
                if (MOMENTS) sab += (unsigned long long)(64 * q + rr) * (unsigned long long)nij;
            }
        }
    }
    mi = wave_sum(mi);
    if (lane == 0) out[4 * q + w] = mi;
    // entropies: label j of a is row j of the histogram -- block j / 64 holds its marginal (thread j % 64); label j of b: block 0
    double ha = 0.0, hb = 0.0;
    if (j < 64 && pa[j] > 0) ha = ((double)pa[j] / N) * (log((double)pa[j]) - logN);
    if (q == 0 && pbj > 0) hb = ((double)pbj / N) * (log((double)pbj) - logN);
    // the single block summed ha over its waves 0 .. 3 = labels 0 .. 255 in runs of 64: here run q is wave 0 of block q
    ha = wave_sum(ha);
    hb = wave_sum(hb);
    if (lane == 0) {
        if (w == 0) out[16 + q] = ha;
        if (q == 0) out[20 + w] = hb;
    }
    if (j == 0) {
        out[24 + q] = (double)cnt[0];
        if (q == 0) out[28] = (double)cnt[1];
    }
    if (MOMENTS) {
        // integer moments (exact: every sum is < 2^32 * 255^2 < 2^48)
        if (sab) atomicAdd(&sm[2], sab * (unsigned long long)j);
        if (j < 64 && pa[j] > 0) {
            const unsigned long long ai = 64 * q + j;
            atomicAdd(&sm[0], ai * pa[j]);
            atomicAdd(&sm[1], ai * ai * pa[j]);
        }
        if (q == 0 && pbj > 0) {
            atomicAdd(&sm[3], (unsigned long long)j * pbj);
            atomicAdd(&sm[4], (unsigned long long)j * j * pbj);
        }
        __syncthreads();
        if (j < NR_MOM) mom[j] = sm[j];
    }
}

// ---- wave partials -> score ---------------------------------------------------------------------------------------------
// p: the NR_PART partials of one histogram
__device__ __forceinline__ double nmi_final_score(const double* __restrict__ p)
{
    const int ca = (int)(p[24] + p[25] + p[26] + p[27]), cb = (int)p[28];
    if (ca == 1 && cb == 1) return 1.0;      // both label sets have a single value
    double tot[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 16; i++) tot[0] += p[i];
    for (int i = 0; i < 4; i++) { tot[1] += p[16 + i]; tot[2] += p[20 + i]; }
    double m = tot[0] < 0 ? 0.0 : tot[0];
    if (fabs(m) < DBL_EPSILON) return 0.0;
    double h_a = ca == 1 ? 0.0 : -tot[1], h_b = cb == 1 ? 0.0 : -tot[2];
    double norm = 0.5 * (h_a + h_b);
    if (norm < DBL_EPSILON) norm = DBL_EPSILON;
    return m / norm;
}
