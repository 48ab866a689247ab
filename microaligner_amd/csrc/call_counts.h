// The event counts that a call returns beside its result (unsupported, dropped, not_converged, folded, ...), stated once:
// how the threads of a kernel tally them and how a C entry keeps them in the ctx workspace and reads them back
// (flow_smooth.hip, flow_median.hip, flow_fill.hip, flow_invert.hip; flow_refine.hip for the host side, local_norm.hip for
// the wave tally: its four counters are those of window_fir.h's wf_acquire).  Off the measured
// path: nothing in register() or warp() reaches it (a header of single sources, build.SOURCE_HEADERS).
//
// Integer adds only, so the totals do not depend on the order in which the waves arrive: two calls give the same counts.
// fr_col_kernel (flow_refine.hip) keeps a tree of its own: its third value is a maximum (atomicMax).
// Other reductions, not this one: fg_error_kernel (flow_grid.hip: per cell, an LDS stage and a maximum), qc.hip (min / max
// partials over all threads of a block) and the per-cell class counter of tx_col_kernel / lc_col_kernel (window_fir.h).
#pragma once
#include "ma_internal.h"

namespace {

// counts[k] += the wave's total of c[k], k < N: a shuffle tree over the 64 lanes, then one atomic of lane 0 per value that
// is not zero.  Every lane of the wave must reach the call (a thread without work brings zeros; no early return before
// it).  counts must not be NULL: where the counts are optional the caller tests the pointer, which is wave-uniform.
template <int N>
__device__ __forceinline__ void d_wave_tally(unsigned long long* counts, const unsigned (&c)[N])
{
    unsigned v[N];
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = c[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] += __shfl_down(v[k], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++)
            if (v[k]) atomicAdd(counts + k, (unsigned long long)v[k]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The device counters of a call, n of them and zeroed on the stream, if the caller asked for counts (else NULL).  They are
// the first bytes of the ctx workspace, and ctx->ws moves when the workspace grows: take them after the call's last
// ma_ws_reserve.  A call that keeps more in the workspace reserves all of it first and lays the rest out behind them.
inline int ma_call_counts(ma_ctx* ctx, bool wanted, int n, unsigned long long** counts)
{
    *counts = nullptr;
    if (!wanted) return MA_OK;
    MA_TRY(ma_ws_reserve(ctx, n * sizeof(unsigned long long)));
    MA_TRY(ma_pinned_reserve(ctx, n * sizeof(unsigned long long)));
    *counts = (unsigned long long*)ctx->ws;
    MA_HIP(hipMemsetAsync(*counts, 0, n * sizeof(unsigned long long), ctx->stream));
    return MA_OK;
}

// host[0 .. n) = the counters, behind everything enqueued on the ctx stream; synchronises
inline int ma_read_call_counts(ma_ctx* ctx, const unsigned long long* counts, int n, long long* host)
{
    MA_HIP(hipMemcpyAsync(ctx->pinned, counts, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    MA_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++) host[k] = (long long)((const unsigned long long*)ctx->pinned)[k];
    return MA_OK;
}

} // namespace
