// Evaluation of a grid flow (include/microaligner_flowgrid.h) inside a kernel: the axis arithmetic, the node patch of a
// block's tile staged in LDS, and E at a pixel of the tile.  Shared by flow_grid.hip (expand, loss), warp_compose.hip (the
// warp from a grid) and flow_invert.hip (the float64 point sampler).  Off the measured path: a header of single sources
// (build.SOURCE_HEADERS).
//
// A tile of FG_TILE_W columns by TH rows needs the nodes of the cells its pixels lie in: at most FG_TILE_W / s + 2 columns
// and TH / s + 2 rows, FG_TILE_W + 1 by TH + 1 with s = 1.  The block stages them once, together with every tile row's
// patch row and ty; a thread keeps its column's patch column and tx in registers, so a pixel costs one 8-byte and four
// 16-byte-at-most LDS reads (the row entry is the same address for the whole wave: a broadcast) and the fourteen
// multiplies and adds of E, no integer or float division.
#pragma once
#include "ma_internal.h"

constexpr int FG_TILE_W = 64, FG_PATCH_W = FG_TILE_W + 2;

struct FgGrid {
    const float2* __restrict__ nodes;   // (gh, gw)
    int H, W, s, gh, gw;
};

// g(n, s); s <= 2^30 and n <= 2^30 keep every k * s below 2^31
__host__ __device__ inline int fg_nodes(int n, int s) { return n <= 1 ? 1 : (n - 2) / s + 2; }

// the grid of an (H, W) flow at stride s: a stride above the longer side means the same as that side
inline FgGrid fg_grid(const float* nodes, int H, int W, int s)
{
    const int m = H > W ? H : W;
    s = s < m ? s : m;
    return FgGrid{(const float2*)nodes, H, W, s, fg_nodes(H, s), fg_nodes(W, s)};
}

struct FgCell {
    int i;      // cell of the pixel
    float t;    // weight of the cell's second node
};

__device__ __forceinline__ FgCell fg_cell(int x, int n, int s, int g)
{
    if (g < 2) return FgCell{0, 0.f};
    const int i = min(x / s, g - 2), p0 = i * s, p1 = min(p0 + s, n - 1);
    return FgCell{i, __fdiv_rn((float)(x - p0), (float)(p1 - p0))};
}

struct __attribute__((aligned(8))) FgRow {
    int j;       // patch row of the cell's upper nodes
    float ty;
};

template <int TH>
struct FgTile {                     // lives in LDS
    float2 n[TH + 1][FG_PATCH_W];   // the node patch
    FgRow row[TH];                  // per tile row
};

struct FgCol {      // a thread's column
    int c, dc;      // patch column of the cell's left nodes; 1, or 0 on a one-node axis
    float tx, bx;   // weight of the right nodes, 1 - tx
};

// Stage what the pixels [x0, x1) x [y0, y1) need (0 < x1 - x0 <= FG_TILE_W, 0 < y1 - y0 <= TH); every thread of the block
// calls it, between two barriers of the caller's.
template <int TH>
__device__ __forceinline__ void fg_stage(FgTile<TH>& t, const FgGrid& g, int x0, int x1, int y0, int y1, int tid, int nt)
{
    const int ci0 = fg_cell(x0, g.W, g.s, g.gw).i, ci1 = min(fg_cell(x1 - 1, g.W, g.s, g.gw).i + 1, g.gw - 1);
    const int cj0 = fg_cell(y0, g.H, g.s, g.gh).i, cj1 = min(fg_cell(y1 - 1, g.H, g.s, g.gh).i + 1, g.gh - 1);
    const int pw = ci1 - ci0 + 1, ph = cj1 - cj0 + 1;
    for (int k = tid; k < pw * ph; k += nt) {
        const int r = k / pw, c = k - r * pw;
        t.n[r][c] = g.nodes[(size_t)(cj0 + r) * g.gw + (ci0 + c)];
    }
    for (int r = tid; r < y1 - y0; r += nt) {
        const FgCell c = fg_cell(y0 + r, g.H, g.s, g.gh);
        t.row[r] = FgRow{c.i - cj0, c.t};
    }
}

// the column state of pixel column x (clamped into the image) in a tile whose first column is x0
__device__ __forceinline__ FgCol fg_col(const FgGrid& g, int x0, int x)
{
    const FgCell c = fg_cell(min(x, g.W - 1), g.W, g.s, g.gw);
    return FgCol{c.i - fg_cell(x0, g.W, g.s, g.gw).i, g.gw > 1 ? 1 : 0, c.t, 1.f - c.t};
}

// E at tile row r of the thread's column
template <int TH>
__device__ __forceinline__ float2 fg_eval(const FgTile<TH>& t, const FgGrid& g, const FgCol& col, int r)
{
    const FgRow e = t.row[r];
    const int j = e.j, j1 = j + (g.gh > 1 ? 1 : 0);
    const float ty = e.ty, by = 1.f - ty;
    const float2 n00 = t.n[j][col.c], n01 = t.n[j][col.c + col.dc], n10 = t.n[j1][col.c], n11 = t.n[j1][col.c + col.dc];
    const float topx = n00.x * col.bx + n01.x * col.tx, botx = n10.x * col.bx + n11.x * col.tx;
    const float topy = n00.y * col.bx + n01.y * col.tx, boty = n10.y * col.bx + n11.y * col.tx;
    return make_float2(topx * by + botx * ty, topy * by + boty * ty);
}

// ---- float64 point sampler G64 ----------------------------------------------------------------------------------------
__device__ __forceinline__ void fg_cell64(double c, int n, int s, int g, int& i, int& i1, double& t)
{
    if (g < 2) { i = i1 = 0; t = 0.0; return; }
    i = min((int)floor(c) / s, g - 2);
    i1 = i + 1;
    const int p0 = i * s, p1 = min(p0 + s, n - 1);
    t = (c - (double)p0) / (double)(p1 - p0);
}

struct FgSampler64 {
    FgGrid g;
    __device__ __forceinline__ double2 operator()(double mx, double my) const
    {
        const double cx = fmin(fmax(mx, 0.0), (double)(g.W - 1)), cy = fmin(fmax(my, 0.0), (double)(g.H - 1));
        int i, i1, j, j1;
        double tx, ty;
        fg_cell64(cx, g.W, g.s, g.gw, i, i1, tx);
        fg_cell64(cy, g.H, g.s, g.gh, j, j1, ty);
        const double bx = 1.0 - tx, by = 1.0 - ty;
        const float2* r0 = g.nodes + (size_t)j * g.gw;
        const float2* r1 = g.nodes + (size_t)j1 * g.gw;
        const float2 n00 = r0[i], n01 = r0[i1], n10 = r1[i], n11 = r1[i1];
        const double topx = (double)n00.x * bx + (double)n01.x * tx, botx = (double)n10.x * bx + (double)n11.x * tx;
        const double topy = (double)n00.y * bx + (double)n01.y * tx, boty = (double)n10.y * bx + (double)n11.y * tx;
        return make_double2(topx * by + botx * ty, topy * by + boty * ty);
    }
};
