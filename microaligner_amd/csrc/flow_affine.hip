// The least-squares moments of a flow's affine part and the re-expression of a flow relative to a matrix
// (include/microaligner_flowaffine.h).  Off the measured path: nothing in register() or warp() calls it.
//
// Moments: one streaming pass, the geometry of qc_flow_tile_kernel without its halo and without LDS rows.  A block covers a
// tile of FA_TW columns x FA_TH rows of one cell and walks down it row by row; a lane owns one 16-byte pair of pixels of
// the flow's memory per row (the pair index is that of the memory, not of the tile, so the load is aligned whatever the
// row's start) and loads it whole where the pair lies inside the row's span, pixel by pixel (8 B) at its ends.  FA_TW = 510:
// any span of 510 pixels touches at most 256 pairs.  The 14 sums and 4 counts stay in registers (float64, every operation
// its own rounding), are combined over the block and written as the tile's partial; fa_cell_kernel adds the partials of a
// cell.  Both in the fixed order of moment_sums.h: two calls give the same bits.
// Apply: pointwise, 8 B in and 8 B out per pixel.
#include "../../include/microaligner_flowaffine.h"
#include "cell_grid.h"
#include "moment_sums.h"
#include "weight_map.h"

#include <cmath>

namespace {

constexpr int FA_SIDE_MAX = 1 << 24;
constexpr int FA_T = 256, FA_TW = 510, FA_TH = 64;
constexpr int FA_NS = MA_FLOW_AFFINE_SUMS, FA_NC = MA_FLOW_AFFINE_COUNTS;

struct FaPart {                 // a tile's partial, and a cell's result
    double s[FA_NS];
    unsigned long long c[FA_NC];
};

struct FaPrior {
    double t[6], clip;
};

struct FaAcc {
    double s[FA_NS];
    unsigned used, invalid, unweighted, trimmed;
};

// one pixel of the header's section 1; wgt is weight(p)
template <bool TRIM>
__device__ __forceinline__ void fa_pixel(FaAcc& acc, int x, int y, double cx, double cy, float2 f, float wgt, const FaPrior& pr)
{
    if (!(d_finite(f.x) && d_finite(f.y))) {
        acc.invalid++;
        return;
    }
    if (!d_weight_counts(wgt)) {
        acc.unweighted++;
        return;
    }
    const double X = __dsub_rn((double)x, cx), Y = __dsub_rn((double)y, cy);
    const double u = (double)f.x, v = (double)f.y;
    const double a = __dsub_rn(X, u), b = __dsub_rn(Y, v);
    if (TRIM) {
        const double rx = __dsub_rn(X, __dadd_rn(__dadd_rn(__dmul_rn(pr.t[0], a), __dmul_rn(pr.t[1], b)), pr.t[2]));
        const double ry = __dsub_rn(Y, __dadd_rn(__dadd_rn(__dmul_rn(pr.t[3], a), __dmul_rn(pr.t[4], b)), pr.t[5]));
        if (!(fabs(rx) <= pr.clip && fabs(ry) <= pr.clip)) {
            acc.trimmed++;
            return;
        }
    }
    acc.used++;
    const double w = (double)wgt;
    const double wa = __dmul_rn(w, a), wb = __dmul_rn(w, b);
    const double t[FA_NS] = {w, wa, wb, __dmul_rn(wa, a), __dmul_rn(wa, b), __dmul_rn(wb, b),
                             __dmul_rn(w, X), __dmul_rn(w, Y), __dmul_rn(wa, X), __dmul_rn(wb, X), __dmul_rn(wa, Y),
                             __dmul_rn(wb, Y), __dmul_rn(__dmul_rn(w, u), u), __dmul_rn(__dmul_rn(w, v), v)};
#pragma unroll
    for (int k = 0; k < FA_NS; k++) acc.s[k] = __dadd_rn(acc.s[k], t[k]);
}

template <int KIND, bool TRIM>
__global__ __launch_bounds__(FA_T) void fa_tile_kernel(const float* __restrict__ flow, MaCellGrid g, const void* __restrict__ weight,
                                                       int ntx, int ntiles, int vec_ok, FaPrior pr, FaPart* __restrict__ part)
{
    __shared__ FaPart red[FA_T / 64];
    int cy0, cy1, cx0, cx1;
    g.rect(g.cell0 + blockIdx.y, cy0, cy1, cx0, cx1);
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x0 = cx0 + tx * FA_TW, y0 = cy0 + ty * FA_TH;
    FaPart* out = part + (size_t)blockIdx.y * ntiles + blockIdx.x;
    if (x0 >= cx1 || y0 >= cy1) {          // outside a ragged cell: the neutral partial
        if (threadIdx.x == 0) *out = FaPart{};
        return;
    }
    const int x1 = min(x0 + FA_TW, cx1), y1 = min(y0 + FA_TH, cy1);
    const int W = g.w;
    const double cx = (double)(W - 1) * 0.5, cy = (double)(g.h - 1) * 0.5;
    // the per-cell weight: the cells of the map are the cells of this call, so a block reads one entry
    const float cell_w = KIND == MA_SMOOTH_WEIGHT_CELLS ? ((const float*)weight)[g.cell0 + blockIdx.y] : 1.f;
    auto weight_at = [&](size_t i) -> float { return KIND == MA_SMOOTH_WEIGHT_CELLS ? cell_w : d_weight_px(weight, KIND, i); };

    FaAcc acc{};
    for (int y = y0; y < y1; y++) {
        const size_t row = (size_t)y * W;
        const size_t L0 = row + x0, L1 = row + x1;
        const size_t p0 = 2 * ((L0 >> 1) + threadIdx.x);      // pixel pair p0, p0 + 1 of the flow's memory
        if (p0 >= L1) continue;
        if (vec_ok && p0 >= L0 && p0 + 2 <= L1) {
            const float4 f = *(const float4*)(flow + 2 * p0);
            const int x = (int)(p0 - row);
            fa_pixel<TRIM>(acc, x, y, cx, cy, make_float2(f.x, f.y), weight_at(p0), pr);
            fa_pixel<TRIM>(acc, x + 1, y, cx, cy, make_float2(f.z, f.w), weight_at(p0 + 1), pr);
        } else {
            for (size_t p = p0; p < p0 + 2; p++)
                if (p >= L0 && p < L1)
                    fa_pixel<TRIM>(acc, (int)(p - row), y, cx, cy, *(const float2*)(flow + 2 * p), weight_at(p), pr);
        }
    }
    FaPart v;
#pragma unroll
    for (int k = 0; k < FA_NS; k++) v.s[k] = acc.s[k];
    v.c[0] = acc.used; v.c[1] = acc.invalid; v.c[2] = acc.unweighted; v.c[3] = acc.trimmed;
    v = d_moments_block<FA_T>(red, v);
    if (threadIdx.x == 0) *out = v;
}

// per cell (blockIdx.x): the tiles' partials in a fixed order
__global__ __launch_bounds__(FA_T) void fa_cell_kernel(const FaPart* __restrict__ part, int ntiles, FaPart* __restrict__ res)
{
    __shared__ FaPart red[FA_T / 64];
    FaPart v{};
    for (int i = threadIdx.x; i < ntiles; i += FA_T) {
        const FaPart p = part[(size_t)blockIdx.x * ntiles + i];
#pragma unroll
        for (int k = 0; k < FA_NS; k++) v.s[k] = __dadd_rn(v.s[k], p.s[k]);
#pragma unroll
        for (int k = 0; k < FA_NC; k++) v.c[k] += p.c[k];
    }
    v = d_moments_block<FA_T>(red, v);
    if (threadIdx.x == 0) res[blockIdx.x] = v;
}

struct FaMat { double a[6]; };

// flow and out may be one array: neither is __restrict__, and a thread reads flow only at the pixel it writes.
__global__ __launch_bounds__(256) void fa_apply_kernel(const float2* flow, int W, int nbx, FaMat m, float2* out)
{
    const int x = (int)(blockIdx.x % nbx) * 256 + threadIdx.x;
    const int y = (int)(blockIdx.x / nbx);
    if (x >= W) return;
    const size_t i = (size_t)y * W + x;
    const float2 f = flow[i];
    const double px = (double)x, py = (double)y;
    const double qx = __dsub_rn(px, (double)f.x), qy = __dsub_rn(py, (double)f.y);
    const double rx = __dadd_rn(__dadd_rn(__dmul_rn(m.a[0], qx), __dmul_rn(m.a[1], qy)), m.a[2]);
    const double ry = __dadd_rn(__dadd_rn(__dmul_rn(m.a[3], qx), __dmul_rn(m.a[4], qy)), m.a[5]);
    out[i] = make_float2((float)__dsub_rn(px, rx), (float)__dsub_rn(py, ry));
}

template <int KIND>
static void fa_launch(ma_ctx* ctx, const float* flow, const MaCellGrid& g, const void* weight, int ntx, int ntiles, unsigned nb,
                      int vec_ok, bool trim, const FaPrior& pr, FaPart* part)
{
    if (trim)
        hipLaunchKernelGGL((fa_tile_kernel<KIND, true>), dim3((unsigned)ntiles, nb), dim3(FA_T), 0, ctx->stream, flow, g, weight,
                           ntx, ntiles, vec_ok, pr, part);
    else
        hipLaunchKernelGGL((fa_tile_kernel<KIND, false>), dim3((unsigned)ntiles, nb), dim3(FA_T), 0, ctx->stream, flow, g, weight,
                           ntx, ntiles, vec_ok, pr, part);
}

} // namespace

extern "C" int ma_flow_affine_moments(ma_ctx* ctx, const float* flow, int H, int W, const void* weight, int weight_kind,
                                      int cell_h, int cell_w, const double* prior, double clip, double* sums_host,
                                      long long* counts_host)
{
    MA_REQUIRE(ctx && flow && sums_host && counts_host, "NULL argument");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FA_SIDE_MAX && W <= FA_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_TRY(ma_weight_check(weight, weight_kind, true, {}, cell_h, cell_w));   // writes host arrays only
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    FaPrior pr{};
    if (prior) {
        for (int k = 0; k < 6; k++) {
            MA_REQUIRE(std::isfinite(prior[k]), "the prior must be finite");
            pr.t[k] = prior[k];
        }
        MA_REQUIRE(clip > 0.0, "clip must be > 0 with a prior");
        pr.clip = clip;
    }
    MaCellGrid g;
    long long ncells;
    MA_TRY(ma_cell_grid(H, W, cell_h, cell_w, &g, &ncells));
    const int ntx = (g.cw + FA_TW - 1) / FA_TW;
    const long long ntiles = (long long)ntx * ((g.ch + FA_TH - 1) / FA_TH);
    MA_REQUIRE(ntiles <= 0x7fffffff, "cell too large");
    const int vec_ok = ((size_t)flow & 15) == 0 ? 1 : 0;
    return ma_cell_batches(
        ctx, ncells, (size_t)(ntiles + 1) * sizeof(FaPart), sizeof(FaPart), 65535,
        [&](long long c0, unsigned nb, const void** dev, size_t* bytes) -> int {
            FaPart* part = (FaPart*)ctx->ws;
            FaPart* res = part + (size_t)nb * ntiles;
            g.cell0 = c0;
            MaProfScope ps(ctx, MA_K_OTHER, (double)H * W * ((double)nb / ncells));
            ma_weight_dispatch(weight_kind, [&](auto kind) {
                fa_launch<kind()>(ctx, flow, g, weight, ntx, (int)ntiles, nb, vec_ok, prior != nullptr, pr, part);
            });
            hipLaunchKernelGGL(fa_cell_kernel, dim3(nb), dim3(FA_T), 0, ctx->stream, (const FaPart*)part, (int)ntiles, res);
            MA_HIP(hipGetLastError());
            *dev = res;
            *bytes = (size_t)nb * sizeof(FaPart);
            return MA_OK;
        },
        [&](long long c0, unsigned nb, const void* pinned) {
            ma_moments_scatter((const FaPart*)pinned, c0, nb, sums_host, counts_host);
        });
}

extern "C" int ma_flow_affine_apply(ma_ctx* ctx, const float* flow, int H, int W, const double* a, float* out)
{
    MA_REQUIRE(ctx && flow && a && out, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FA_SIDE_MAX && W <= FA_SIDE_MAX, "flow sides must be in [1, 2^24]");
    FaMat m;
    for (int k = 0; k < 6; k++) {
        MA_REQUIRE(std::isfinite(a[k]), "the matrix must be finite");
        m.a[k] = a[k];
    }
    const long long nbx = (W + 255) / 256;
    MA_REQUIRE(nbx * H <= 0x7fffffffLL, "flow too large");
    MA_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(fa_apply_kernel, dim3((unsigned)(nbx * H)), dim3(256), 0, ctx->stream, (const float2*)flow, W, (int)nbx, m,
                       (float2*)out);
    MA_HIP(hipGetLastError());
    return MA_OK;
}
