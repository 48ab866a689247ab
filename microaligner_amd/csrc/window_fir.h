// The separable window FIR behind the flow smoothing, the texture maps, the flow refinement, the local correlation maps and
// the local contrast normalisation (flow_smooth.hip, texture.hip, flow_refine.hip, local_correlation.hip, local_norm.hip): its tile, stated once.  Off the measured path: nothing in register() or warp() reaches it (a header of
// single sources, build.SOURCE_HEADERS).
//
// A symmetric FIR with up to 2 * WF_MAX_RADIUS + 1 taps over P planes, in two launches through a workspace of 4 P B/px that
// holds the row pass's planes TRANSPOSED ((W, H) each).  Both passes are then the same tile: 64 lines (lanes) x WF_S = WF_NW *
// WF_R outputs along the filtered axis, which is the fast axis of what the pass reads.
//   - staging: a wave reads a line's span (outputs + r halo + guards) with consecutive lanes on consecutive elements
//     (coalesced: loads of the user's arrays in the row pass, float loads of a transposed plane in the column pass) into
//     LDS [64 lines][pitch], pitch odd, so that these writes and the filter's reads (lane = line) are free of bank conflicts;
//   - filter: a thread slides a register window along its line for WF_R consecutive outputs (d_sym_fir_slide_pk, the
//     window blurs' and DOG's filter), in the accumulation order of the users' headers, one plane after the other through the
//     same LDS tile;
//   - output: lane = line, and a line of the input is a column of the output, so the stores are coalesced as well: the row
//     pass writes its planes transposed, the column pass ends in the user's own epilogue and writes row-major.
// What is stated here: the tile's constants, the tap table and its setup, one plane of a row pass (wf_row_plane) and the host
// side of a call: the tap check, the shape of the launches, and the pool buffers of a call with their unwinding and the
// read-back of per-cell counts (wf_acquire, wf_finish).  The weight that three of the users take is weight_map.h, the
// per-call counts of the smoothing and the refinement call_counts.h.  The column kernels, and the row kernel of the flow smoothing, stage and filter in their own bodies,
// in the words of wf_row_plane: they were compiled as one body, and taken out into a function they compile to other code.
// So does the per-cell class counter of tx_col_kernel and lc_col_kernel (the `while (todo)` loop with the ballots): as one
// templated function it changed 1395 of the 12552 lines of texture.hip's device assembly and 4602 of local_correlation.hip's.
// One kernel family for every r in 1 .. 128: LDS is sized by r at launch (40 KiB at r = 12, 97 KiB at r = 128).
// Bound by the instructions it issues (two LDS reads and three packed operations per tap and 16 outputs), like the window
// blurs, not by bytes; at large r the halo (2r staged elements beside 128 outputs per line) adds to it.
#pragma once
#include "ma_internal.h"

#include <cmath>

namespace {

constexpr int WF_NW = 8, WF_R = 16, WF_S = WF_NW * WF_R;   // waves per block, outputs per thread, outputs per line and block
constexpr int WF_G = 2;                                     // guard elements either side of the halo (d_sym_fir_slide_pk)
constexpr int WF_MAX_RADIUS = 128;
constexpr int WF_TAPS = 8 + WF_MAX_RADIUS + 8;              // floats of a tap table in the MA_TAP layout

// elements of a staged line, and the pitch of the lines in LDS (the kernels state both in place)
inline int wf_span(int r) { return WF_S + 2 * r + 2 * WF_G; }
inline int wf_pitch(int r) { return wf_span(r) | 1; }

struct WfTaps { float t[WF_MAX_RADIUS + 1]; };   // k[0 .. r], the rest 0; passed to a setup kernel by value

// element i < WF_TAPS of the taps in the MA_TAP layout
__device__ __forceinline__ void wf_layout_tap(const WfTaps& taps, int r, int i, float* __restrict__ aux)
{
    float v = 0.f;
    if (i == 0) v = taps.t[0];
    else if (i >= 8 && i - 7 <= r) v = taps.t[i - 7];
    aux[i] = v;
}

// aux[0 .. WF_TAPS): the taps in the MA_TAP layout; one block.  A template only so that a source with a setup kernel of its
// own (flow_smooth.hip) does not carry this one.
template <int = 0>
__global__ __launch_bounds__(256) void wf_setup_kernel(WfTaps taps, int r, float* __restrict__ aux)
{
    if (threadIdx.x < WF_TAPS) wf_layout_tap(taps, r, threadIdx.x, aux);
}

// One plane of the row pass through the block's LDS tile [64][pitch].  Block: rows [y0, y0 + 64) x output columns
// [x0, x0 + WF_S); lane = row, wv = wave (wave-uniform).  at(H, W, x, y): the plane's value at a pixel inside the image,
// outside it the value is 0; H and W reach it from here, so that the compiler knows them for those of the guard.
// dst: the plane's (W, H) array.
template <class At>
__device__ __forceinline__ void wf_row_plane(At at, int H, int W, int r, const float* __restrict__ taps, int x0, int y0,
                                             int lane, int wv, float* lds, float* __restrict__ dst)
{
    const int span = WF_S + 2 * r + 2 * WF_G, pitch = span | 1;
    for (int row = wv; row < 64; row += WF_NW) {
        const int y = y0 + row;
        float* line = lds + row * pitch;
        for (int c = lane; c < span; c += 64) {
            const int x = x0 - r - WF_G + c;
            line[c] = (y < H && x >= 0 && x < W) ? at(H, W, x, y) : 0.f;
        }
    }
    __syncthreads();
    float acc[WF_R];
    d_sym_fir_slide_pk<WF_R, false, false>(lds + lane * pitch, WF_G + r + wv * WF_R, r, taps, acc);
    __syncthreads();
    const int y = y0 + lane;
#pragma unroll
    for (int q = 0; q < WF_R; q++) {
        const int x = x0 + wv * WF_R + q;
        if (x < W && y < H) dst[(size_t)x * H + y] = acc[q];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the caller's taps k[0 .. r], checked
inline int wf_taps(const float* host, int r, WfTaps* taps)
{
    *taps = WfTaps{};
    for (int k = 0; k <= r; k++) {
        MA_REQUIRE(std::isfinite(host[k]) && host[k] >= 0.f, "taps must be finite and not negative");
        taps->t[k] = host[k];
    }
    MA_REQUIRE(taps->t[0] > 0.f, "the centre tap must be positive");
    return MA_OK;
}

// blocks of a 1-D grid over nbx x nby tiles; what: "flow" or "image", for the refusal
inline int wf_grid(long long nbx, long long nby, const char* what, unsigned* blocks)
{
    if (nbx * nby > 0x7fffffffLL) {
        ma_set_error("invalid argument: %s too large", what);
        return MA_EINVAL;
    }
    *blocks = (unsigned)(nbx * nby);
    return MA_OK;
}

// how the two passes over an (H, W) image are launched at radius r: 64 * WF_NW threads, lds bytes of dynamic LDS
struct WfShape {
    size_t lds;
    int nbx_row, nbx_col;      // tiles along x of the row and of the column pass (the kernels' nbx)
    unsigned g_row, g_col;     // blocks
};

// the shape, and the opt-in of the row and the column kernel to its LDS where that is above 64 KiB
inline int wf_shape(int H, int W, int r, const char* what, const void* row, const void* col, WfShape* s)
{
    s->lds = (size_t)64 * wf_pitch(r) * sizeof(float);
    s->nbx_row = (W + WF_S - 1) / WF_S;
    s->nbx_col = (W + 63) / 64;
    MA_TRY(wf_grid(s->nbx_row, (H + 63) / 64, what, &s->g_row));
    MA_TRY(wf_grid(s->nbx_col, (H + WF_S - 1) / WF_S, what, &s->g_col));
    if (s->lds > 64 * 1024) {
        MA_HIP(hipFuncSetAttribute(row, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->lds));
        MA_HIP(hipFuncSetAttribute(col, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->lds));
    }
    return MA_OK;
}

// The pool buffers of a call: aux (the tap table and `tail` floats behind it), the workspace of `planes` (W, H) planes and,
// for the maps with per-cell class counts, n zeroed counters (n = 0: none).
struct WfBuffers {
    float* aux;
    float* ws;
    unsigned long long* counts;
    size_t n;
};

// Ends a call: with rc == MA_OK and counters, reads them straight into the caller's array (unsigned on the device, the same
// bits as the long long asked for) and synchronises; then frees in the order counts, ws, aux.  -> the first error.
// Stream-ordered reuse: the next call on this ctx that takes the buffers runs behind the kernels launched here.
inline int wf_finish(ma_ctx* ctx, const WfBuffers& b, int rc, long long* counts_host)
{
    if (rc == MA_OK && b.counts) {
        hipError_t e = hipMemcpyAsync(counts_host, b.counts, b.n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ma_set_error("reading the class counts failed: %s", hipGetErrorString(e));
            rc = MA_EHIP;
        }
    }
    if (b.counts) ma_pool_free(ctx, b.counts);
    if (b.ws) ma_pool_free(ctx, b.ws);
    if (b.aux) ma_pool_free(ctx, b.aux);
    return rc;
}

// Takes the buffers, the memset of the counters first on the stream; on failure frees what it took.
inline int wf_acquire(ma_ctx* ctx, size_t tail, int planes, int H, int W, size_t n, WfBuffers* b)
{
    *b = WfBuffers{nullptr, nullptr, nullptr, n};
    b->aux = (float*)ma_pool_alloc(ctx, ((size_t)WF_TAPS + tail) * sizeof(float));
    if (b->aux) b->ws = (float*)ma_pool_alloc(ctx, (size_t)H * W * planes * sizeof(float));
    if (b->ws && n) b->counts = (unsigned long long*)ma_pool_alloc(ctx, n * sizeof(unsigned long long));
    if (!b->ws || (n && !b->counts)) return wf_finish(ctx, *b, MA_ENOMEM, nullptr);
    if (n && hipMemsetAsync(b->counts, 0, n * sizeof(unsigned long long), ctx->stream) != hipSuccess) {
        ma_set_error("hipMemsetAsync of the class counts failed");
        return wf_finish(ctx, *b, MA_EHIP, nullptr);
    }
    return MA_OK;
}

} // namespace
