// The cell grid of the per-cell maps (qc.hip, residual_shift.hip) and the loop that walks it in batches of cells.  Off the
// measured path: nothing in register() or warp() reaches it (a header of single sources, build.SOURCE_HEADERS).
//
// Cells: a grid from (0, 0) of ch x cw pixels over an (h, w) image, gx columns of cells, the last row / column ragged; cells
// are numbered row-major.
#pragma once
#include "ma_internal.h"

struct MaCellGrid {
    int h, w, ch, cw, gx;
    long long cell0;   // first cell of the batch (row-major cell index)

    __device__ __forceinline__ void rect(long long cell, int& y0, int& y1, int& x0, int& x1) const
    {
        const int ci = (int)(cell / gx), cj = (int)(cell % gx);
        y0 = ci * ch;
        y1 = min(y0 + ch, h);
        x0 = cj * cw;
        x1 = min(x0 + cw, w);
    }
};

__device__ __forceinline__ bool ma_finite(double x) { return x - x == 0.0; }

// the grid of cell_h x cell_w cells over an (h, w) image (cell0 = 0) and its number of cells
inline int ma_cell_grid(int h, int w, int cell_h, int cell_w, MaCellGrid* g, long long* ncells)
{
    MA_REQUIRE(h > 0 && w > 0, "empty image");
    MA_REQUIRE(cell_h > 0 && cell_w > 0, "cell size must be >= 1");
    const int ch = cell_h < h ? cell_h : h, cw = cell_w < w ? cell_w : w;   // a larger cell is the whole axis
    *g = MaCellGrid{h, w, ch, cw, (w + cw - 1) / cw, 0};
    *ncells = (long long)((h + ch - 1) / ch) * g->gx;
    return MA_OK;
}

// the same grid as the struct of a kernel that counts per cell takes it (o->ch, o->cw, o->gx)
template <class Out>
int ma_cell_counts_grid(int h, int w, int cell_h, int cell_w, Out* o, long long* ncells)
{
    MaCellGrid g;
    MA_TRY(ma_cell_grid(h, w, cell_h, cell_w, &g, ncells));
    o->ch = g.ch;
    o->cw = g.cw;
    o->gx = g.gx;
    return MA_OK;
}

// All cells in batches of at most `cap`, sized so that ws_per bytes of the device workspace per cell stay within the ctx's
// workspace limit.  Per batch: enqueue(c0, nb, &dev, &bytes) launches the work of the cells [c0, c0 + nb) on the ctx stream
// and names the device span that holds their results (at most pin_per bytes per cell); the span is copied to ctx->pinned,
// the stream synchronised and scatter(c0, nb, pinned) writes the caller's arrays.
template <class Enqueue, class Scatter>
int ma_cell_batches(ma_ctx* ctx, long long ncells, size_t ws_per, size_t pin_per, long long cap, Enqueue enqueue,
                    Scatter scatter)
{
    long long batch = (long long)(ctx->ws_limit / ws_per);
    if (batch > ncells) batch = ncells;
    if (batch > cap) batch = cap;
    if (batch < 1) {
        ma_set_error("workspace limit %zu is below the %zu bytes one cell takes", ctx->ws_limit, ws_per);
        return MA_ENOMEM;
    }
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ma_ws_reserve(ctx, (size_t)batch * ws_per));
    MA_TRY(ma_pinned_reserve(ctx, (size_t)batch * pin_per));
    for (long long c0 = 0; c0 < ncells; c0 += batch) {
        const unsigned nb = (unsigned)(ncells - c0 < batch ? ncells - c0 : batch);
        const void* dev = nullptr;
        size_t bytes = 0;
        MA_TRY(enqueue(c0, nb, &dev, &bytes));
        MA_HIP(hipMemcpyAsync(ctx->pinned, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MA_HIP(hipStreamSynchronize(ctx->stream));
        scatter(c0, nb, (const void*)ctx->pinned);
    }
    if (ctx->profile) MA_TRY(ma_profile_flush(ctx));
    return MA_OK;
}
