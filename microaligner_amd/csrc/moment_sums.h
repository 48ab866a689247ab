// The fixed-order float64 reduction of the moment sums (flow_affine.hip, direct_affine.hip), stated once.  Off the measured
// path: nothing in register() or warp() reaches it (a header of single sources, build.SOURCE_HEADERS).
//
// A partial P is any struct with the members `double s[]` (sums) and `unsigned long long c[]` (counts); FaPart and DaPart are
// two plain structs, not one template: the template's arguments would enter the mangled name of every kernel that takes a
// partial.  Every float64 add is its own rounding (__dadd_rn) and happens at a fixed place of a fixed tree: the lanes of a
// wave by shuffles, the waves of a block in sequence, the tiles of a cell in sequence per thread and then the same block
// tree.  No floating-point atomics: two calls give the same bits.
// What is stated here: the block tree (d_moments_block) and the host's scatter of the results.  The loop before the tree in
// fa_cell_kernel and da_final_kernel (thread t adds the partials t, t + NT, ... in that order) stays in their bodies: as one
// function (a pointer or an offset to the first partial, the index as int or as unsigned) both compile to other code: the
// operands of the count adds change places and fa_cell_kernel addresses its loads from another base.
#pragma once
#include "ma_internal.h"

namespace {

template <class P>
struct MomentSizes {
    static constexpr int NS = (int)(sizeof(P::s) / sizeof(double)), NC = (int)(sizeof(P::c) / sizeof(unsigned long long));
};

// The block's total of v in a fixed order: the lanes of a wave by a shuffle tree, then the waves 0, 1, ... in sequence by
// thread 0.  Valid in thread 0.  NT: threads of the block, all of which must reach the call; red: one P per wave, in LDS.
template <int NT, class P>
__device__ __forceinline__ P d_moments_block(P* red, P v)
{
    constexpr int NS = MomentSizes<P>::NS, NC = MomentSizes<P>::NC;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NS; k++) v.s[k] = __dadd_rn(v.s[k], __shfl_down(v.s[k], off, 64));
#pragma unroll
        for (int k = 0; k < NC; k++) v.c[k] += __shfl_down(v.c[k], off, 64);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int wv = 1; wv < NT / 64; wv++) {
#pragma unroll
            for (int k = 0; k < NS; k++) v.s[k] = __dadd_rn(v.s[k], red[wv].s[k]);
#pragma unroll
            for (int k = 0; k < NC; k++) v.c[k] += red[wv].c[k];
        }
    return v;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the results r[0 .. nb) of the cells c0, c0 + 1, ... into the caller's arrays of NS sums and NC counts per cell
template <class P>
inline void ma_moments_scatter(const P* r, long long c0, unsigned nb, double* sums_host, long long* counts_host)
{
    constexpr int NS = MomentSizes<P>::NS, NC = MomentSizes<P>::NC;
    for (unsigned i = 0; i < nb; i++) {
        for (int k = 0; k < NS; k++) sums_host[(size_t)(c0 + i) * NS + k] = r[i].s[k];
        for (int k = 0; k < NC; k++) counts_host[(size_t)(c0 + i) * NC + k] = (long long)r[i].c[k];
    }
}

} // namespace
