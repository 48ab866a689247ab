// Grid flows (include/microaligner_flowgrid.h): the nodes of a flow, their expansion and the loss maps of a (flow, nodes)
// pair.  Off the measured path: nothing in register() or warp() calls it.
//
// Expansion and loss share flow_grid_eval.h's tile: a block of 256 threads covers 64 columns by 32 rows, stages the tile's
// node patch and row weights in LDS once, and a thread evaluates FG_R rows of one column.  The loss is a float32 maximum
// (taken on the bits: e >= 0 and never NaN, so the unsigned order is the float order) and two integer counts, reduced per
// wave, then per block, then with one atomic each into the cell's accumulators: independent of every order.
#include "cell_grid.h"
#include "flow_grid_eval.h"
#include "../../include/microaligner_flowgrid.h"

#include <cmath>

namespace {

constexpr int FG_SIDE_MAX = 1 << 24;
constexpr int FG_WAVES = 4, FG_R = 8, FG_TH = FG_WAVES * FG_R;

__global__ __launch_bounds__(256) void fg_sample_kernel(const float2* __restrict__ flow, FgGrid g, float2* __restrict__ nodes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.gw) return;
    const int px = min(i * g.s, g.W - 1);
    for (int j = blockIdx.y; j < g.gh; j += gridDim.y) {
        const int py = min(j * g.s, g.H - 1);
        nodes[(size_t)j * g.gw + i] = flow[(size_t)py * g.W + px];
    }
}

__global__ __launch_bounds__(256) void fg_expand_kernel(FgGrid g, int nty, float2* __restrict__ out)
{
    __shared__ FgTile<FG_TH> tile;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int x0 = blockIdx.x * FG_TILE_W, x1 = min(x0 + FG_TILE_W, g.W), x = x0 + lane;
    const FgCol col = fg_col(g, x0, x);
    // more tile rows than gridDim.y holds: a block strides over them (every thread of it alike)
    for (int ty = blockIdx.y; ty < nty; ty += gridDim.y) {
        const int y0 = ty * FG_TH, y1 = min(y0 + FG_TH, g.H);
        __syncthreads();      // the tile before is read
        fg_stage(tile, g, x0, x1, y0, y1, (int)threadIdx.x, 256);
        __syncthreads();
        if (x >= g.W) continue;
#pragma unroll
        for (int r = 0; r < FG_R; r++) {
            const int y = y0 + wave * FG_R + r;
            if (y < y1) out[(size_t)y * g.W + x] = fg_eval(tile, g, col, wave * FG_R + r);
        }
    }
}

struct FgAcc {
    unsigned max_bits, pad;            // bits of the float32 maximum of e plus 1; 0: no valid pixel yet
    unsigned long long above, invalid;
};

// blockIdx.x = tile of the geometry of a full cell, blockIdx.y = cell of the batch
__global__ __launch_bounds__(256) void fg_error_kernel(const float2* __restrict__ flow, FgGrid g, MaCellGrid cg, int ntx,
                                                       float tol, FgAcc* __restrict__ acc)
{
    __shared__ FgTile<FG_TH> tile;
    __shared__ unsigned s_max[FG_WAVES], s_above[FG_WAVES], s_inv[FG_WAVES];
    int cy0, cy1, cx0, cx1;
    cg.rect(cg.cell0 + blockIdx.y, cy0, cy1, cx0, cx1);
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x0 = cx0 + tx * FG_TILE_W, y0 = cy0 + ty * FG_TH;
    if (x0 >= cx1 || y0 >= cy1) return;       // a ragged cell: the whole block leaves
    const int x1 = min(x0 + FG_TILE_W, cx1), y1 = min(y0 + FG_TH, cy1);
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int x = x0 + lane;
    const FgCol col = fg_col(g, x0, x);
    fg_stage(tile, g, x0, x1, y0, y1, (int)threadIdx.x, 256);
    __syncthreads();
    unsigned mx = 0, above = 0, inv = 0;      // a thread sees at most FG_R pixels
    if (x < x1) {
#pragma unroll
        for (int r = 0; r < FG_R; r++) {
            const int y = y0 + wave * FG_R + r;
            if (y >= y1) break;
            const float2 e = fg_eval(tile, g, col, wave * FG_R + r), f = flow[(size_t)y * g.W + x];
            const float dx = e.x - f.x, dy = e.y - f.y;
            if (dx != dx || dy != dy) {
                inv++;
            } else {
                const float err = fmaxf(fabsf(dx), fabsf(dy));
                mx = max(mx, __float_as_uint(err) + 1u);   // + 1: zero stays "no valid pixel"; Inf's bits + 1 do not wrap
                above += err > tol ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mx = max(mx, (unsigned)__shfl_down(mx, off, 64));
        above += __shfl_down(above, off, 64);
        inv += __shfl_down(inv, off, 64);
    }
    if (lane == 0) { s_max[wave] = mx; s_above[wave] = above; s_inv[wave] = inv; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < FG_WAVES; k++) { mx = max(mx, s_max[k]); above += s_above[k]; inv += s_inv[k]; }
        FgAcc* a = acc + blockIdx.y;
        if (mx) atomicMax(&a->max_bits, mx);
        if (above) atomicAdd(&a->above, (unsigned long long)above);
        if (inv) atomicAdd(&a->invalid, (unsigned long long)inv);
    }
}

int check_grid(int H, int W, int s)
{
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FG_SIDE_MAX && W <= FG_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(s >= 1, "the stride must be at least 1");
    return MA_OK;
}

} // namespace

extern "C" {

int ma_flow_grid_sample(ma_ctx* ctx, const float* flow, int H, int W, int s, float* nodes)
{
    MA_REQUIRE(ctx && flow && nodes, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(nodes, 8, "nodes");
    MA_TRY(check_grid(H, W, s));
    const FgGrid g = fg_grid(nullptr, H, W, s);
    MA_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(fg_sample_kernel, dim3((g.gw + 255) / 256, std::min(g.gh, MA_GRID_Y_MAX)), dim3(256), 0, ctx->stream,
                       (const float2*)flow, g, (float2*)nodes);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

int ma_flow_grid_expand(ma_ctx* ctx, const float* nodes, int H, int W, int s, float* out)
{
    MA_REQUIRE(ctx && nodes && out, "NULL argument");
    MA_REQUIRE_ALIGNED(nodes, 8, "nodes");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_TRY(check_grid(H, W, s));
    const FgGrid g = fg_grid(nodes, H, W, s);
    const int nty = (H + FG_TH - 1) / FG_TH;
    MA_HIP(hipSetDevice(ctx->device));
    MaProfScope ps(ctx, MA_K_OTHER, (double)H * W);
    hipLaunchKernelGGL(fg_expand_kernel, dim3((W + FG_TILE_W - 1) / FG_TILE_W, std::min(nty, MA_GRID_Y_MAX)), dim3(256), 0,
                       ctx->stream, g, nty, (float2*)out);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

int ma_flow_grid_error(ma_ctx* ctx, const float* flow, const float* nodes, int H, int W, int s, int cell_h, int cell_w,
                       float tol, float* max_err, long long* above, long long* invalid)
{
    MA_REQUIRE(ctx && flow && nodes && max_err && above && invalid, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(nodes, 8, "nodes");
    MA_TRY(check_grid(H, W, s));
    MA_REQUIRE(tol == tol, "tol must not be NaN");
    MaCellGrid cg;
    long long ncells;
    MA_TRY(ma_cell_grid(H, W, cell_h, cell_w, &cg, &ncells));
    const FgGrid g = fg_grid(nodes, H, W, s);
    const int ntx = (cg.cw + FG_TILE_W - 1) / FG_TILE_W;
    const long long ntiles = (long long)ntx * ((cg.ch + FG_TH - 1) / FG_TH);   // <= 2^18 * 2^19
    MA_REQUIRE(ntiles <= 0x7fffffff, "cell too large");
    return ma_cell_batches(
        ctx, ncells, sizeof(FgAcc), sizeof(FgAcc), MA_GRID_Y_MAX,
        [&](long long c0, unsigned nb, const void** dev, size_t* bytes) -> int {
            FgAcc* acc = (FgAcc*)ctx->ws;
            cg.cell0 = c0;
            MA_HIP(hipMemsetAsync(acc, 0, (size_t)nb * sizeof(FgAcc), ctx->stream));
            MaProfScope ps(ctx, MA_K_OTHER, (double)H * W * ((double)nb / ncells));
            hipLaunchKernelGGL(fg_error_kernel, dim3((unsigned)ntiles, nb), dim3(256), 0, ctx->stream, (const float2*)flow, g, cg,
                               ntx, tol, acc);
            MA_HIP(hipGetLastError());
            *dev = acc;
            *bytes = (size_t)nb * sizeof(FgAcc);
            return MA_OK;
        },
        [&](long long c0, unsigned nb, const void* pinned) {
            const FgAcc* a = (const FgAcc*)pinned;
            for (unsigned i = 0; i < nb; i++) {
                const unsigned bits = a[i].max_bits ? a[i].max_bits - 1u : 0x7fc00000u;   // no valid pixel: NaN
                float v;
                __builtin_memcpy(&v, &bits, 4);
                max_err[c0 + i] = v;
                above[c0 + i] = (long long)a[i].above;
                invalid[c0 + i] = (long long)a[i].invalid;
            }
        });
}

} // extern "C"
