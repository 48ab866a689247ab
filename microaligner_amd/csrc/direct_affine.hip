// The Gauss-Newton moments of the intensity-based affine alignment (include/microaligner_direct.h).  Off the measured
// path: nothing in register() or warp() calls it.
//
// One streaming pass over the reference, the scheme of fa_tile_kernel (flow_affine.hip): a block covers a tile of DA_TW
// columns x DA_TH rows and walks down it row by row, a lane owns one column, so the reference (and the weight) is read
// coalesced and the four taps of a wave's row are gathers that stay within a few rows of the moving image for a small
// rotation.  The gradient is that of the bilinear interpolant itself: no neighbours, no LDS tile.  The 31 sums and 5 counts
// stay in registers (float64, every operation its own rounding), are combined over the block and written as the tile's
// partial; da_final_kernel adds the partials.  Both in the fixed order of moment_sums.h: two calls give the same bits.  The
// host side is the batch loop of cell_grid.h with the image as its one cell.
#include "../../include/microaligner_direct.h"
#include "cell_grid.h"
#include "moment_sums.h"
#include "weight_map.h"

#include <cmath>

namespace {

constexpr int DA_SIDE_MAX = 1 << 24;
constexpr int DA_T = 256, DA_TW = 256, DA_TH = 64;
constexpr int DA_NS = MA_DIRECT_AFFINE_SUMS, DA_NC = MA_DIRECT_AFFINE_COUNTS;

struct DaPart {                 // a tile's partial, and the result
    double s[DA_NS];
    unsigned long long c[DA_NC];
};

struct DaArgs {
    double m[6], gain, bias, clip;
    int H, W, ntx, weight_kind, trim;
};

template <typename T>
__device__ __forceinline__ bool da_finite(T) { return true; }
template <>
__device__ __forceinline__ bool da_finite<float>(float v) { return fabsf(v) < INFINITY; }

// counts: used, outside, invalid, unweighted, trimmed
enum { DA_USED = 0, DA_OUTSIDE = 1, DA_INVALID = 2, DA_UNWEIGHTED = 3, DA_TRIMMED = 4 };

template <typename TR, typename TM>
__global__ __launch_bounds__(DA_T) void da_tile_kernel(const TR* __restrict__ ref, const TM* __restrict__ mov,
                                                       const void* __restrict__ weight, DaArgs a, DaPart* __restrict__ part)
{
    __shared__ DaPart red[DA_T / 64];
    const int W = a.W, H = a.H;
    const int x = (int)(blockIdx.x % (unsigned)a.ntx) * DA_TW + (int)threadIdx.x;
    const int y0 = (int)(blockIdx.x / (unsigned)a.ntx) * DA_TH, y1 = min(y0 + DA_TH, H);
    const double cx = (double)(W - 1) * 0.5, cy = (double)(H - 1) * 0.5;
    const double xmax = (double)(W - 2), ymax = (double)(H - 2);

    double s[DA_NS];
#pragma unroll
    for (int k = 0; k < DA_NS; k++) s[k] = 0.0;
    unsigned cnt[DA_NC] = {0, 0, 0, 0, 0};

    if (x < W) {
        const double px = (double)x;
        const double X = __dsub_rn(px, cx), XX = __dmul_rn(X, X);
        const double m0x = __dmul_rn(a.m[0], px), m3x = __dmul_rn(a.m[3], px);
        for (int y = y0; y < y1; y++) {
            const double py = (double)y;
            const double sx = __dadd_rn(__dadd_rn(m0x, __dmul_rn(a.m[1], py)), a.m[2]);
            const double sy = __dadd_rn(__dadd_rn(m3x, __dmul_rn(a.m[4], py)), a.m[5]);
            const double fx = floor(sx), fy = floor(sy);
            const bool inside = fx >= 0.0 && fx <= xmax && fy >= 0.0 && fy <= ymax;      // a NaN fails
            const size_t i = (size_t)y * W + x;
            // the classes are worked out without branches and the sums are added under one, so that the 31 accumulators are
            // not copied where branches merge
            TR vi = (TR)0;
            TM v00 = (TM)0, v01 = (TM)0, v10 = (TM)0, v11 = (TM)0;
            float wgt = 1.f;
            if (inside) {
                // 0 <= fx <= W - 2, 0 <= fy <= H - 2: all four taps exist
                const size_t q = (size_t)(int)fy * W + (size_t)(int)fx;
                vi = ref[i];
                v00 = mov[q], v01 = mov[q + 1], v10 = mov[q + W], v11 = mov[q + W + 1];
                wgt = d_weight_px(weight, a.weight_kind, i);
            }
            const bool finite = da_finite(vi) && da_finite(v00) && da_finite(v01) && da_finite(v10) && da_finite(v11);
            const bool weighted = d_weight_counts(wgt);
            const double tx = __dsub_rn(sx, fx), ty = __dsub_rn(sy, fy);
            const double a00 = (double)v00, a01 = (double)v01, a10 = (double)v10, a11 = (double)v11;
            const double d0 = __dsub_rn(a01, a00), d1 = __dsub_rn(a11, a10);
            const double top = __dadd_rn(a00, __dmul_rn(d0, tx)), bot = __dadd_rn(a10, __dmul_rn(d1, tx));
            const double gy = __dsub_rn(bot, top);
            const double m = __dadd_rn(top, __dmul_rn(gy, ty));
            const double gx = __dadd_rn(d0, __dmul_rn(__dsub_rn(d1, d0), ty));
            const double I = (double)vi;
            const double e = __dsub_rn(I, __dadd_rn(__dmul_rn(a.gain, m), a.bias));
            const bool kept = !(a.trim && !(fabs(e) <= a.clip));
            // each pixel in exactly one class, tested in the header's order
            const bool invalid = inside && !finite, unweighted = inside && finite && !weighted;
            const bool trimmed = inside && finite && weighted && !kept, used = inside && finite && weighted && kept;
            cnt[DA_OUTSIDE] += !inside;
            cnt[DA_INVALID] += invalid;
            cnt[DA_UNWEIGHTED] += unweighted;
            cnt[DA_TRIMMED] += trimmed;
            if (!used) continue;
            cnt[DA_USED]++;
            const double w = (double)wgt;
            const double Y = __dsub_rn(py, cy);
            const double XY = __dmul_rn(X, Y), YY = __dmul_rn(Y, Y);
            const double wgx = __dmul_rn(w, gx), wgy = __dmul_rn(w, gy);
            const double A[3] = {__dmul_rn(wgx, gx), __dmul_rn(wgx, gy), __dmul_rn(wgy, gy)};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s[6 * k + 0] = __dadd_rn(s[6 * k + 0], __dmul_rn(A[k], XX));
                s[6 * k + 1] = __dadd_rn(s[6 * k + 1], __dmul_rn(A[k], XY));
                s[6 * k + 2] = __dadd_rn(s[6 * k + 2], __dmul_rn(A[k], X));
                s[6 * k + 3] = __dadd_rn(s[6 * k + 3], __dmul_rn(A[k], YY));
                s[6 * k + 4] = __dadd_rn(s[6 * k + 4], __dmul_rn(A[k], Y));
                s[6 * k + 5] = __dadd_rn(s[6 * k + 5], A[k]);
            }
            const double we = __dmul_rn(w, e);
            const double ex = __dmul_rn(we, gx), ey = __dmul_rn(we, gy);
            s[18] = __dadd_rn(s[18], __dmul_rn(ex, X));
            s[19] = __dadd_rn(s[19], __dmul_rn(ex, Y));
            s[20] = __dadd_rn(s[20], ex);
            s[21] = __dadd_rn(s[21], __dmul_rn(ey, X));
            s[22] = __dadd_rn(s[22], __dmul_rn(ey, Y));
            s[23] = __dadd_rn(s[23], ey);
            s[24] = __dadd_rn(s[24], __dmul_rn(we, e));
            const double wm = __dmul_rn(w, m), wI = __dmul_rn(w, I);
            s[25] = __dadd_rn(s[25], w);
            s[26] = __dadd_rn(s[26], wm);
            s[27] = __dadd_rn(s[27], wI);
            s[28] = __dadd_rn(s[28], __dmul_rn(wm, m));
            s[29] = __dadd_rn(s[29], __dmul_rn(wm, I));
            s[30] = __dadd_rn(s[30], __dmul_rn(wI, I));
        }
    }
    DaPart v;
#pragma unroll
    for (int k = 0; k < DA_NS; k++) v.s[k] = s[k];
#pragma unroll
    for (int k = 0; k < DA_NC; k++) v.c[k] = cnt[k];
    v = d_moments_block<DA_T>(red, v);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// one block: the tiles' partials in a fixed order
__global__ __launch_bounds__(DA_T) void da_final_kernel(const DaPart* __restrict__ part, int ntiles, DaPart* __restrict__ res)
{
    __shared__ DaPart red[DA_T / 64];
    DaPart v{};
    for (unsigned i = threadIdx.x; i < (unsigned)ntiles; i += DA_T) {      // ntiles <= 2^31 - 1: no wrap
        const DaPart p = part[i];
#pragma unroll
        for (int k = 0; k < DA_NS; k++) v.s[k] = __dadd_rn(v.s[k], p.s[k]);
#pragma unroll
        for (int k = 0; k < DA_NC; k++) v.c[k] += p.c[k];
    }
    v = d_moments_block<DA_T>(red, v);
    if (threadIdx.x == 0) *res = v;
}

// out = mask != 0 ? 1 : 0, four pixels a thread where they are whole
__global__ __launch_bounds__(256) void da_mask_kernel(const unsigned char* __restrict__ mask, size_t n, float* __restrict__ out)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (i + k < n) out[i + k] = mask[i + k] ? 1.f : 0.f;
}

template <typename TR>
static void da_launch(ma_ctx* ctx, const void* ref, const void* mov, int mov_dtype, const void* weight, const DaArgs& a,
                      unsigned ntiles, DaPart* part)
{
    switch (mov_dtype) {
    case MA_U8: hipLaunchKernelGGL((da_tile_kernel<TR, unsigned char>), dim3(ntiles), dim3(DA_T), 0, ctx->stream, (const TR*)ref, (const unsigned char*)mov, weight, a, part); break;
    case MA_U16: hipLaunchKernelGGL((da_tile_kernel<TR, unsigned short>), dim3(ntiles), dim3(DA_T), 0, ctx->stream, (const TR*)ref, (const unsigned short*)mov, weight, a, part); break;
    default: hipLaunchKernelGGL((da_tile_kernel<TR, float>), dim3(ntiles), dim3(DA_T), 0, ctx->stream, (const TR*)ref, (const float*)mov, weight, a, part); break;
    }
}

} // namespace

extern "C" int ma_direct_affine_moments(ma_ctx* ctx, const void* ref, int ref_dtype, const void* mov, int mov_dtype, int H, int W,
                                        const double* M, double gain, double bias, const void* weight, int weight_kind,
                                        double clip, double* sums_host, long long* counts_host)
{
    MA_REQUIRE(ctx && ref && mov && M && sums_host && counts_host, "NULL argument");
    MA_REQUIRE(ref_dtype >= MA_U8 && ref_dtype <= MA_F32 && mov_dtype >= MA_U8 && mov_dtype <= MA_F32, "unknown dtype");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= DA_SIDE_MAX && W <= DA_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_TRY(ma_weight_check(weight, weight_kind, false, {}, 1, 1));   // writes host arrays only
    DaArgs a{};
    for (int k = 0; k < 6; k++) {
        MA_REQUIRE(std::isfinite(M[k]), "the matrix must be finite");
        a.m[k] = M[k];
    }
    MA_REQUIRE(std::isfinite(gain) && std::isfinite(bias), "gain and bias must be finite");
    a.gain = gain; a.bias = bias;
    a.trim = clip > 0.0 ? 1 : 0;          // a NaN is no clipping
    a.clip = a.trim ? clip : 0.0;
    a.H = H; a.W = W; a.weight_kind = weight_kind;
    a.ntx = (W + DA_TW - 1) / DA_TW;
    const long long ntiles = (long long)a.ntx * ((H + DA_TH - 1) / DA_TH);
    MA_REQUIRE(ntiles <= 0x7fffffff, "image too large");
    // the whole image is one cell: the tiles' partials and, behind them, the result
    return ma_cell_batches(
        ctx, 1, (size_t)(ntiles + 1) * sizeof(DaPart), sizeof(DaPart), 1,
        [&](long long, unsigned, const void** dev, size_t* bytes) -> int {
            DaPart* part = (DaPart*)ctx->ws;
            DaPart* res = part + ntiles;
            MaProfScope ps(ctx, MA_K_OTHER, (double)H * W);
            switch (ref_dtype) {
            case MA_U8: da_launch<unsigned char>(ctx, ref, mov, mov_dtype, weight, a, (unsigned)ntiles, part); break;
            case MA_U16: da_launch<unsigned short>(ctx, ref, mov, mov_dtype, weight, a, (unsigned)ntiles, part); break;
            default: da_launch<float>(ctx, ref, mov, mov_dtype, weight, a, (unsigned)ntiles, part); break;
            }
            hipLaunchKernelGGL(da_final_kernel, dim3(1), dim3(DA_T), 0, ctx->stream, (const DaPart*)part, (int)ntiles, res);
            MA_HIP(hipGetLastError());
            *dev = res;
            *bytes = sizeof(DaPart);
            return MA_OK;
        },
        [&](long long c0, unsigned nb, const void* pinned) {
            ma_moments_scatter((const DaPart*)pinned, c0, nb, sums_host, counts_host);
        });
}

extern "C" int ma_direct_mask_weight(ma_ctx* ctx, const unsigned char* mask, size_t n, float* out)
{
    MA_REQUIRE(ctx && mask && out, "NULL argument");
    MA_REQUIRE(n >= 1 && n <= (size_t)0x7fffffff * 1024, "the mask holds 1 to (2^31 - 1) * 1024 pixels");
    const size_t nb = (n + 1023) / 1024;
    MA_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(da_mask_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, mask, n, out);
    MA_HIP(hipGetLastError());
    return MA_OK;
}
