// Registration quality maps (include/microaligner_qc.h): per-cell NMI / NCC of label images against a reference, and
// per-cell Jacobian and magnitude statistics of a flow.  Off the measured path: nothing in register() or warp() calls it.
//
// The NMI of a cell is the gate's score of the cell's pixels, computed by the gate's own code (nmi_score.h): the same
// 256 x 256 joint histogram, the same f64 formula in the same reduction order, so a cell gives the bits ma_nmi_u8 gives for
// the cropped cell.
#include "cell_grid.h"
#include "flow_jacobian.h"
#include "nmi_score.h"
#include "../../include/microaligner_qc.h"

#include <cmath>

namespace {

// ---- joint histograms of 2-D cells ----------------------------------------------------------------------------------
// A block holds the 256 x 256 histogram of one slice in LDS as the packed 16-bit counters of nmi_score.h (128 KiB), a
// slice of at most HIST_SLICE16 pixels.  Here a slice is a rectangle of a cell: the cell's columns are cut into n_seg
// segments of at most seg_w <= HIST_SLICE16 columns (rows wider than a slice), each segment into runs of
// rows_per = HIST_SLICE16 / seg_w rows.  blockIdx.x = slice (segment + n_seg * row run), blockIdx.y = cell of the batch,
// blockIdx.z = label image (b0 / b1, sharing `a`).  Slices of the geometry of a full cell that fall outside a ragged cell
// are empty.  Work items are 16-byte blocks of the image memory within one row of the slice, so a lane reads 16
// consecutive pixels with one 16-byte load per array where the block lies wholly inside the row (decorrelating the bins of
// neighbouring lanes on smooth images, as in nmi.hip) and byte by byte at the row ends.
constexpr long long QC_BATCH = 2048;

template <int NT>
__global__ __launch_bounds__(NT) void qc_joint_hist_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b0,
                                                           const uint8_t* __restrict__ b1, MaCellGrid g, int seg_w, int n_seg,
                                                           int rows_per, int vec_ok, unsigned* __restrict__ hist)
{
    extern __shared__ unsigned h[];              // [256 * 256 / 2]
    const uint8_t* __restrict__ b = blockIdx.z ? b1 : b0;
    int cy0, cy1, cx0, cx1;
    g.rect(g.cell0 + blockIdx.y, cy0, cy1, cx0, cx1);
    const int seg = blockIdx.x % n_seg, rs = blockIdx.x / n_seg;
    const int x0 = cx0 + seg * seg_w, y0 = cy0 + rs * rows_per;
    if (x0 >= cx1 || y0 >= cy1) return;
    const int x1 = min(x0 + seg_w, cx1), y1 = min(y0 + rows_per, cy1);
    hist16_zero<NT, 32768>(h);
    __syncthreads();
    auto count = [&](unsigned ai, unsigned bi) { hist16_add(h, ai, bi); };
    const int nbm = (x1 - x0 + 15) / 16 + 1;    // 16-byte blocks a row of the slice touches, at most
    const int items = (y1 - y0) * nbm;
    for (int t = threadIdx.x; t < items; t += NT) {
        const int r = t / nbm, k = t - r * nbm;
        const size_t row = (size_t)(y0 + r) * (size_t)g.w;
        const size_t lo = row + x0, hi = row + x1;
        const size_t base = ((lo >> 4) + (size_t)k) << 4;
        if (base >= hi) continue;
        if (vec_ok && base >= lo && base + 16 <= hi) {
            const uint4 av = *(const uint4*)(a + base), bv = *(const uint4*)(b + base);
            const unsigned aw[4] = {av.x, av.y, av.z, av.w}, bw[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int q = 0; q < 16; q++)
                count((aw[q >> 2] >> ((q & 3) * 8)) & 255u, (bw[q >> 2] >> ((q & 3) * 8)) & 255u);
        } else {
            const size_t e = base + 16 < hi ? base + 16 : hi;
            for (size_t i = base > lo ? base : lo; i < e; i++) count(a[i], b[i]);
        }
    }
    __syncthreads();
    hist16_flush<NT, 32768>(h, hist + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * 65536);
}

// The gate's score per cell (nmi_reduce_block): N is the cell's number of pixels; besides the wave partials each block leaves
// the integer moments of its rows for the Pearson correlation.
__global__ __launch_bounds__(NR_T) void qc_score_reduce_kernel(const unsigned* __restrict__ hist, MaCellGrid g, unsigned ncells,
                                                               double* __restrict__ part, unsigned long long* __restrict__ mom)
{
    int cy0, cy1, cx0, cx1;
    g.rect(g.cell0 + blockIdx.x % ncells, cy0, cy1, cx0, cx1);
    const double N = (double)((size_t)(cy1 - cy0) * (size_t)(cx1 - cx0));
    nmi_reduce_block<true>(hist + (size_t)blockIdx.x * 65536, N, part + (size_t)blockIdx.x * NR_PART,
                           mom + ((size_t)blockIdx.x * NR_Q + blockIdx.y) * NR_MOM);
}

// scores[b] = NMI, scores[nhist + b] = Pearson r of histogram b
__global__ __launch_bounds__(64) void qc_score_final_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ mom,
                                                            MaCellGrid g, unsigned ncells, unsigned nhist, double* __restrict__ scores)
{
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nhist) return;
    scores[b] = nmi_final_score(part + (size_t)b * NR_PART);

    unsigned long long s[NR_MOM] = {0, 0, 0, 0, 0};
    for (int q = 0; q < NR_Q; q++)
        for (int k = 0; k < NR_MOM; k++) s[k] += mom[((size_t)b * NR_Q + q) * NR_MOM + k];
    int cy0, cy1, cx0, cx1;
    g.rect(g.cell0 + b % ncells, cy0, cy1, cx0, cx1);
    const __int128 n = (__int128)((long long)(cy1 - cy0) * (long long)(cx1 - cx0));
    const __int128 sa = s[0], saa = s[1], sab = s[2], sb = s[3], sbb = s[4];
    const __int128 cov = n * sab - sa * sb, va = n * saa - sa * sa, vb = n * sbb - sb * sb;
    double r;
    if (va <= 0 || vb <= 0) r = NAN;
    else {
        r = (double)cov / (sqrt((double)va) * sqrt((double)vb));
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    }
    scores[nhist + b] = r;
}

// ---- flow statistics --------------------------------------------------------------------------------------------
// A block covers a tile of QF_TW columns x QF_TH rows of one cell and walks down it row by row.  Row y + 1 (and the one
// column of halo either side) is read into a ring of four LDS rows while rows y - 1 and y are already there, so every flow
// value of the tile is read from HBM once (plus the halo); lanes load two pixels (16 B) where the pair lies inside the
// loaded span, one pixel (8 B) at its ends.  One barrier per row: the ring has four slots, so the slot a fast wave fills
// for row y + 2 is not one a slow wave still reads for row y.
constexpr int QF_T = 256, QF_TW = 508, QF_TH = 64, QF_LW = QF_TW + 2;

struct QcFlowPart {
    double jmin, sum, max;
    unsigned folded, invalid, nfin, pad;
};

template <int NT>
__device__ __forceinline__ void qc_block_combine(QcFlowPart* s, QcFlowPart v)
{
    // fixed-order tree over the block's threads (deterministic)
    s[threadIdx.x] = v;
    __syncthreads();
    for (int st = NT / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            QcFlowPart a = s[threadIdx.x], b = s[threadIdx.x + st];
            a.jmin = fmin(a.jmin, b.jmin);
            a.sum = a.sum + b.sum;
            a.max = fmax(a.max, b.max);
            a.folded += b.folded;
            a.invalid += b.invalid;
            a.nfin += b.nfin;
            s[threadIdx.x] = a;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(QF_T) void qc_flow_tile_kernel(const float* __restrict__ flow, MaCellGrid g, int ntx, int ntiles,
                                                            int vec_ok, QcFlowPart* __restrict__ part)
{
    __shared__ float su[4][QF_LW], sv[4][QF_LW];
    __shared__ QcFlowPart red[QF_T];
    int cy0, cy1, cx0, cx1;
    g.rect(g.cell0 + blockIdx.y, cy0, cy1, cx0, cx1);
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int x0 = cx0 + tx * QF_TW, y0 = cy0 + ty * QF_TH;
    QcFlowPart* out = part + (size_t)blockIdx.y * ntiles + blockIdx.x;
    if (x0 >= cx1 || y0 >= cy1) {          // outside a ragged cell: the neutral partial
        if (threadIdx.x == 0) *out = QcFlowPart{INFINITY, 0.0, -1.0, 0u, 0u, 0u, 0u};
        return;
    }
    const int x1 = min(x0 + QF_TW, cx1), y1 = min(y0 + QF_TH, cy1);
    const int W = g.w, H = g.h;
    const int lx0 = max(x0 - 1, 0), lx1 = min(x1 + 1, W);   // loaded columns (tile + halo inside the image)

    auto load_row = [&](int yy) {
        const size_t L0 = (size_t)yy * W + lx0, L1 = (size_t)yy * W + lx1;
        const size_t P = (L0 >> 1) + threadIdx.x;           // pixel pair 2P, 2P + 1 (<= 256 pairs span the row)
        const size_t p0 = 2 * P;
        if (p0 >= L1) return;
        float* u = su[yy & 3];
        float* v = sv[yy & 3];
        const long long off = (long long)(yy) * W + (x0 - 1);   // LDS column = linear pixel - off
        if (vec_ok && p0 >= L0 && p0 + 2 <= L1) {
            const float4 f = *(const float4*)(flow + 2 * p0);
            u[p0 - off] = f.x; v[p0 - off] = f.y;
            u[p0 + 1 - off] = f.z; v[p0 + 1 - off] = f.w;
        } else {
            for (size_t p = p0; p < p0 + 2; p++)
                if (p >= L0 && p < L1) {
                    const float2 f = *(const float2*)(flow + 2 * p);
                    u[p - off] = f.x; v[p - off] = f.y;
                }
        }
    };

    QcFlowPart acc{INFINITY, 0.0, -1.0, 0u, 0u, 0u, 0u};
    if (y0 > 0) load_row(y0 - 1);
    load_row(y0);
    for (int y = y0; y < y1; y++) {
        if (y + 1 < H) load_row(y + 1);
        __syncthreads();
        const float* um = su[(y + 3) & 3]; const float* vm = sv[(y + 3) & 3];
        const float* uc = su[y & 3];       const float* vc = sv[y & 3];
        const float* up = su[(y + 1) & 3]; const float* vp = sv[(y + 1) & 3];
        for (int x = x0 + threadIdx.x; x < x1; x += QF_T) {
            const int c = x - x0 + 1;
            const double u = uc[c], v = vc[c];
            // det J of flow_jacobian.h from the three LDS rows
            const double det = ma_flow_det_j(
                [&](int dx, int dy) {
                    const float* ur = dy < 0 ? um : (dy > 0 ? up : uc);
                    const float* vr = dy < 0 ? vm : (dy > 0 ? vp : vc);
                    return make_float2(ur[c + dx], vr[c + dx]);
                },
                x, y, W, H);
            if (ma_finite(det)) {
                acc.jmin = fmin(acc.jmin, det);
                acc.folded += det <= 0.0;
            }
            if (ma_finite(u) && ma_finite(v)) {
                const double m = __dsqrt_rn(__dadd_rn(__dmul_rn(u, u), __dmul_rn(v, v)));
                acc.sum = __dadd_rn(acc.sum, m);
                acc.max = fmax(acc.max, m);
                acc.nfin++;
            } else {
                acc.invalid++;
            }
        }
    }
    qc_block_combine<QF_T>(red, acc);
    if (threadIdx.x == 0) *out = red[0];
}

// per cell (blockIdx.x): the tiles' partials in a fixed order -> jac_min, folded, invalid, mean, max
constexpr int QF_RT = 256;
__global__ __launch_bounds__(QF_RT) void qc_flow_cell_kernel(const QcFlowPart* __restrict__ part, int ntiles,
                                                             double* __restrict__ res)
{
    __shared__ double smin[QF_RT], ssum[QF_RT], smax[QF_RT];
    __shared__ unsigned long long sfold[QF_RT], sinv[QF_RT], sfin[QF_RT];
    const int t = threadIdx.x;
    double mn = INFINITY, sum = 0.0, mx = -1.0;
    unsigned long long fold = 0, inv = 0, fin = 0;
    for (int i = t; i < ntiles; i += QF_RT) {
        const QcFlowPart p = part[(size_t)blockIdx.x * ntiles + i];
        mn = fmin(mn, p.jmin);
        sum = sum + p.sum;
        mx = fmax(mx, p.max);
        fold += p.folded; inv += p.invalid; fin += p.nfin;
    }
    smin[t] = mn; ssum[t] = sum; smax[t] = mx; sfold[t] = fold; sinv[t] = inv; sfin[t] = fin;
    __syncthreads();
    for (int st = QF_RT / 2; st > 0; st >>= 1) {
        if (t < st) {
            smin[t] = fmin(smin[t], smin[t + st]);
            ssum[t] = ssum[t] + ssum[t + st];
            smax[t] = fmax(smax[t], smax[t + st]);
            sfold[t] += sfold[t + st]; sinv[t] += sinv[t + st]; sfin[t] += sfin[t + st];
        }
        __syncthreads();
    }
    if (t == 0) {
        double* r = res + (size_t)blockIdx.x * 5;
        r[0] = smin[0];
        r[1] = (double)sfold[0];
        r[2] = (double)sinv[0];
        r[3] = sfin[0] ? ssum[0] / (double)sfin[0] : NAN;
        r[4] = sfin[0] ? smax[0] : NAN;
    }
}

} // namespace

extern "C" {

int ma_qc_nmi_grid(ma_ctx* ctx, const uint8_t* ref, const uint8_t* b0, const uint8_t* b1, int h, int w, int cell_h, int cell_w,
                   double* nmi0_host, double* nmi1_host, double* ncc0_host, double* ncc1_host)
{
    MA_REQUIRE(ctx && ref && b0 && nmi0_host && ncc0_host && (!b1 || (nmi1_host && ncc1_host)), "NULL argument");
    MaCellGrid g;
    long long ncells;
    MA_TRY(ma_cell_grid(h, w, cell_h, cell_w, &g, &ncells));
    MA_REQUIRE((unsigned long long)g.ch * (unsigned long long)g.cw < (1ull << 32), "a cell must hold fewer than 2^32 pixels");
    const unsigned nimg = b1 ? 2 : 1;
    // slice geometry of a full cell: balanced column segments of <= HIST_SLICE16 columns, runs of rows that keep a slice
    // <= HIST_SLICE16
    const int n_seg = (g.cw + HIST_SLICE16 - 1) / HIST_SLICE16;
    const int seg_w = (g.cw + n_seg - 1) / n_seg;
    const int rows_per = HIST_SLICE16 / seg_w;
    const long long slices = (long long)n_seg * ((g.ch + rows_per - 1) / rows_per);
    MA_REQUIRE(slices <= 0x7fffffff, "cell too large");
    // per cell and label image: histogram (256 KiB), wave partials, moments, two scores
    const size_t per = 65536 * sizeof(unsigned) + NR_PART * sizeof(double) + NR_Q * NR_MOM * sizeof(unsigned long long) +
                       2 * sizeof(double);
    const int vec_ok = ((((size_t)ref | (size_t)b0 | (size_t)(b1 ? b1 : b0)) & 15) == 0) ? 1 : 0;
    // at most QC_BATCH cells at a time: the histograms of a batch take 256 KiB per cell and image of the grow-only workspace
    return ma_cell_batches(
        ctx, ncells, per * nimg, nimg * 2 * sizeof(double), QC_BATCH,
        [&](long long c0, unsigned nb, const void** dev, size_t* bytes) -> int {
            const unsigned nhist = nb * nimg;
            unsigned* hist = (unsigned*)ctx->ws;
            double* part = (double*)(hist + (size_t)nhist * 65536);
            unsigned long long* mom = (unsigned long long*)(part + (size_t)nhist * NR_PART);
            double* scores = (double*)(mom + (size_t)nhist * NR_Q * NR_MOM);
            g.cell0 = c0;
            MaProfScope ps(ctx, MA_K_OTHER, (double)h * w * nimg * ((double)nb / ncells));
            MA_HIP(hipMemsetAsync(hist, 0, (size_t)nhist * 65536 * sizeof(unsigned), ctx->stream));
            hipLaunchKernelGGL((qc_joint_hist_kernel<1024>), dim3((unsigned)slices, nb, nimg), dim3(1024), 32768 * sizeof(unsigned),
                               ctx->stream, ref, b0, b1, g, seg_w, n_seg, rows_per, vec_ok, hist);
            hipLaunchKernelGGL(qc_score_reduce_kernel, dim3(nhist, NR_Q), dim3(NR_T), 0, ctx->stream, (const unsigned*)hist, g, nb,
                               part, mom);
            hipLaunchKernelGGL(qc_score_final_kernel, dim3((nhist + 63) / 64), dim3(64), 0, ctx->stream, (const double*)part,
                               (const unsigned long long*)mom, g, nb, nhist, scores);
            MA_HIP(hipGetLastError());
            *dev = scores;
            *bytes = (size_t)2 * nhist * sizeof(double);
            return MA_OK;
        },
        [&](long long c0, unsigned nb, const void* pinned) {
            const double* pin = (const double*)pinned;
            const unsigned nhist = nb * nimg;
            for (unsigned i = 0; i < nb; i++) {
                nmi0_host[c0 + i] = pin[i];
                ncc0_host[c0 + i] = pin[nhist + i];
                if (b1) {
                    nmi1_host[c0 + i] = pin[nb + i];
                    ncc1_host[c0 + i] = pin[nhist + nb + i];
                }
            }
        });
}

int ma_qc_flow_grid(ma_ctx* ctx, const float* flow, int h, int w, int cell_h, int cell_w, double* jac_min_host,
                    long long* folded_host, long long* invalid_host, double* flow_mean_host, double* flow_max_host)
{
    MA_REQUIRE(ctx && flow && jac_min_host && folded_host && invalid_host && flow_mean_host && flow_max_host, "NULL argument");
    MaCellGrid g;
    long long ncells;
    MA_TRY(ma_cell_grid(h, w, cell_h, cell_w, &g, &ncells));
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    const int ntx = (g.cw + QF_TW - 1) / QF_TW;
    const long long ntiles = (long long)ntx * ((g.ch + QF_TH - 1) / QF_TH);
    MA_REQUIRE(ntiles <= 0x7fffffff, "cell too large");
    const int vec_ok = ((size_t)flow & 15) == 0 ? 1 : 0;
    return ma_cell_batches(
        ctx, ncells, (size_t)ntiles * sizeof(QcFlowPart) + 5 * sizeof(double), 5 * sizeof(double), 65535,
        [&](long long c0, unsigned nb, const void** dev, size_t* bytes) -> int {
            QcFlowPart* part = (QcFlowPart*)ctx->ws;
            double* res = (double*)(part + (size_t)nb * ntiles);
            g.cell0 = c0;
            MaProfScope ps(ctx, MA_K_OTHER, (double)h * w * ((double)nb / ncells));
            hipLaunchKernelGGL(qc_flow_tile_kernel, dim3((unsigned)ntiles, nb), dim3(QF_T), 0, ctx->stream, flow, g, ntx,
                               (int)ntiles, vec_ok, part);
            hipLaunchKernelGGL(qc_flow_cell_kernel, dim3(nb), dim3(QF_RT), 0, ctx->stream, (const QcFlowPart*)part, (int)ntiles, res);
            MA_HIP(hipGetLastError());
            *dev = res;
            *bytes = (size_t)nb * 5 * sizeof(double);
            return MA_OK;
        },
        [&](long long c0, unsigned nb, const void* pinned) {
            for (unsigned i = 0; i < nb; i++) {
                const double* r = (const double*)pinned + (size_t)i * 5;
                jac_min_host[c0 + i] = r[0];
                folded_host[c0 + i] = (long long)r[1];
                invalid_host[c0 + i] = (long long)r[2];
                flow_mean_host[c0 + i] = r[3];
                flow_max_host[c0 + i] = r[4];
            }
        });
}

} // extern "C"
