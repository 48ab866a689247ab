// Residual shift maps (include/microaligner_residual.h): per cell, the ZNCC of two u8 label images at every integer shift
// within +-R, its peak and a parabolic sub-pixel refinement.  Off the measured path: nothing in register() or warp()
// calls it.
//
// Every moment is an integer and is summed exactly (u32 inside a tile, u64 beyond), so the table of scores does not depend
// on the tiling, the batching or the order of the atomics; the scores themselves are formed once, in f64, by the finishing
// kernel.
#include "cell_grid.h"
#include "../../include/microaligner_residual.h"

#include <cmath>
#include <cstring>

namespace {

// ---- geometry -----------------------------------------------------------------------------------------------------
// comparison domain of a cell: the cell cut back to [R, h - R) x [R, w - R); empty when oy1 <= oy0 or ox1 <= ox0
__device__ __forceinline__ void rs_domain(const MaCellGrid& g, int R, long long cell, int& oy0, int& oy1, int& ox0, int& ox1)
{
    g.rect(cell, oy0, oy1, ox0, ox1);
    oy0 = max(oy0, R);
    oy1 = min(oy1, g.h - R);
    ox0 = max(ox0, R);
    ox1 = min(ox1, g.w - R);
}

// ---- correlation kernel -----------------------------------------------------------------------------------------------
// A block walks `tpb` tiles of RS_TH rows down one strip of RS_TW columns of a cell's domain.  Per tile it stages, as
// packed bytes in LDS, the tile of `a` (zero outside the domain, so padding adds nothing to any product) and the same
// tile of `b` with a halo of R (zero outside the image; such bytes only ever meet a zero of `a` or a masked lane).
//
//   S_ab : work items are (four consecutive dx of one dy, row group, column segment).  An item walks its rows four pixels at
//          a time: the `a` word is the same for every lane of the item's row (an LDS broadcast); the dword of `b` read in the
//          step before and one new dword give, through v_alignbyte_b32, the `b` words of the four shifts, and four
//          v_dot4_u32_u8 add the products: two LDS reads for sixteen products.  An item makes at most
//          RS_TH * RS_TW / 4 = 1024 steps, far below the 16 512 a u32 holds.
//   S_b, S_bb : box sums of b and b^2 over the tile moved by d.  First the sums of every haloed row over the tile's columns
//          moved by dx (items (row, dx), the same walk with a constant and with b itself as the other operand of the dot),
//          then, per shift, the sum of those over the tile's rows moved by dy.
//
// Tile sums fit u32 (32 * 128 * 255^2 < 2^32); they are added to u64 accumulators in LDS, which the block adds to the
// cell's u64 moments in global memory once, at its end.
constexpr int RS_NT = 256, RS_TW = 128, RS_TH = 32, RS_KW = RS_TW / 4, RS_APD = RS_KW + 1;

struct RsLds {
    int R, D, NS, BR, BPd;           // D = 2R + 1, NS = D * D, BR = RS_TH + 2R rows of b, BPd dwords per row of b
    size_t acc, a, b, hb, hbb, bytes;   // byte offsets
};

RsLds rs_lds_layout(int R)
{
    RsLds L;
    L.R = R; L.D = 2 * R + 1; L.NS = L.D * L.D; L.BR = RS_TH + 2 * R;
    // a row of b holds RS_TW + 2R bytes and one more dword (the walk reads one dword ahead); the lanes of a wave read
    // R / 2 + 1 consecutive dwords of each of several rows at once, so rows start that many banks apart at least
    const int need = R / 2 + 1;
    L.BPd = (RS_TW + 2 * R + 3) / 4 + 1;
    while (L.BPd % 32 < need || L.BPd % 32 > 32 - need) L.BPd++;
    size_t o = 0;
    L.acc = o; o += (size_t)(3 * L.NS + 2) * 8;
    L.a = o; o += (size_t)RS_TH * RS_APD * 4;
    L.b = o; o += (size_t)L.BR * L.BPd * 4;
    L.hb = o; o += (size_t)L.BR * L.D * 4;
    L.hbb = o; o += (size_t)L.BR * L.D * 4;
    L.bytes = o;
    return L;
}

__device__ __forceinline__ unsigned rs_load4(const uint8_t* __restrict__ img, int h, int w, int y, int x, int xlo, int xhi)
{
    // bytes (y, x .. x + 3) of the image as one little-endian word; 0 for every byte outside [xlo, xhi) or the image
    if (y < 0 || y >= h) return 0u;
    const uint8_t* p = img + (size_t)y * (size_t)w;
    if (x >= xlo && x + 4 <= xhi) {
        unsigned v;
        __builtin_memcpy(&v, p + x, 4);
        return v;
    }
    unsigned v = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (x + q >= xlo && x + q < xhi) v |= (unsigned)p[x + q] << (8 * q);
    return v;
}

__global__ __launch_bounds__(RS_NT) void rs_corr_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b0,
                                                        const uint8_t* __restrict__ b1, MaCellGrid g, RsLds L, int nchunk, int tpb,
                                                        int G, int KS, unsigned long long* __restrict__ mom)
{
    extern __shared__ unsigned long long rs_smem[];
    unsigned char* sm = reinterpret_cast<unsigned char*>(rs_smem);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(sm + L.acc);   // [3][NS] S_ab, S_b, S_bb; then S_a, S_aa
    unsigned* A = reinterpret_cast<unsigned*>(sm + L.a);
    unsigned* B = reinterpret_cast<unsigned*>(sm + L.b);
    unsigned* Hb = reinterpret_cast<unsigned*>(sm + L.hb);
    unsigned* Hbb = reinterpret_cast<unsigned*>(sm + L.hbb);

    const uint8_t* __restrict__ b = blockIdx.z ? b1 : b0;
    const int R = L.R, D = L.D, NS = L.NS, BPd = L.BPd, NQ = (D + 3) >> 2;
    int oy0, oy1, ox0, ox1;
    rs_domain(g, R, g.cell0 + blockIdx.y, oy0, oy1, ox0, ox1);
    const int strip = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
    const int tx0 = ox0 + strip * RS_TW;
    const int cy0 = oy0 + chunk * tpb * RS_TH;
    if (oy1 <= oy0 || tx0 >= ox1 || cy0 >= oy1) return;
    const int cy1 = min(cy0 + tpb * RS_TH, oy1);
    const int tw = min(RS_TW, ox1 - tx0);          // valid columns of the strip
    const int kw = (tw + 3) >> 2;                    // words a row walk takes
    const unsigned lastmask = (tw & 3) ? ((1u << (8 * (tw & 3))) - 1u) : 0xffffffffu;
    const int t = threadIdx.x;

    for (int i = t; i < 3 * NS + 2; i += RS_NT) acc[i] = 0ull;
    unsigned sa = 0, saa = 0;     // this thread's share of S_a, S_aa: <= tpb * 4 words * 4 * 255^2, tpb <= 4096 keeps it in u32

    for (int ty0 = cy0; ty0 < cy1; ty0 += RS_TH) {
        const int th = min(RS_TH, cy1 - ty0);
        const int br = th + 2 * R;
        __syncthreads();     // the tile before is done with A and B (and acc is zeroed)
        for (int i = t; i < th * RS_KW; i += RS_NT) {
            const int y = i / RS_KW, k = i - y * RS_KW;
            const unsigned v = rs_load4(a, g.h, g.w, ty0 + y, tx0 + 4 * k, tx0, tx0 + tw);
            A[y * RS_APD + k] = v;
            sa = __builtin_amdgcn_udot4(v, 0x01010101u, sa, false);
            saa = __builtin_amdgcn_udot4(v, v, saa, false);
        }
        for (int i = t; i < br * BPd; i += RS_NT) {
            const int r = i / BPd, c = i - r * BPd;
            B[i] = rs_load4(b, g.h, g.w, ty0 - R + r, tx0 - R + 4 * c, 0, g.w);
        }
        __syncthreads();

        // sums of the haloed rows over the tile's columns moved by dx
        for (int i = t; i < br * D; i += RS_NT) {
            const int r = i / D, o = i - r * D;
            const unsigned* brow = B + r * BPd + (o >> 2);
            const unsigned sh = o & 3;
            unsigned lo = brow[0], s1 = 0, s2 = 0;
            for (int k = 0; k < kw; k++) {
                const unsigned hi = brow[k + 1];
                unsigned bw = __builtin_amdgcn_alignbyte(hi, lo, sh);
                if (k == kw - 1) bw &= lastmask;
                s1 = __builtin_amdgcn_udot4(bw, 0x01010101u, s1, false);
                s2 = __builtin_amdgcn_udot4(bw, bw, s2, false);
                lo = hi;
            }
            Hb[i] = s1;
            Hbb[i] = s2;
        }
        // S_ab: items (column segment, row group, dy, quad of dx), the quad the fastest index so that a wave shares its `a` words
        const int kseg = (kw + KS - 1) / KS;
        for (int i = t; i < NQ * D * G * KS; i += RS_NT) {
            const int q = i % NQ, dy = (i / NQ) % D, grp = (i / (NQ * D)) % G, seg = i / (NQ * D * G);
            const int k0 = seg * kseg, k1 = min(k0 + kseg, kw);
            unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            for (int y = grp; y < th; y += G) {
                const unsigned* arow = A + y * RS_APD;
                const unsigned* brow = B + (y + dy) * BPd + q;
                unsigned lo = k0 < k1 ? brow[k0] : 0u;
#pragma unroll 4
                for (int k = k0; k < k1; k++) {
                    const unsigned hi = brow[k + 1], av = arow[k];
                    s0 = __builtin_amdgcn_udot4(av, lo, s0, false);
                    s1 = __builtin_amdgcn_udot4(av, __builtin_amdgcn_alignbyte(hi, lo, 1u), s1, false);
                    s2 = __builtin_amdgcn_udot4(av, __builtin_amdgcn_alignbyte(hi, lo, 2u), s2, false);
                    s3 = __builtin_amdgcn_udot4(av, __builtin_amdgcn_alignbyte(hi, lo, 3u), s3, false);
                    lo = hi;
                }
            }
            // the last quad of a row of shifts reaches past dx = R: those sums are dropped
            const int o = 4 * q;
            unsigned long long* dst = acc + dy * D + o;
            if (s0) atomicAdd(&dst[0], (unsigned long long)s0);
            if (s1 && o + 1 < D) atomicAdd(&dst[1], (unsigned long long)s1);
            if (s2 && o + 2 < D) atomicAdd(&dst[2], (unsigned long long)s2);
            if (s3 && o + 3 < D) atomicAdd(&dst[3], (unsigned long long)s3);
        }
        __syncthreads();
        // S_b, S_bb of the tile: the row sums over the tile's rows moved by dy (one thread per shift: no atomics)
        for (int s = t; s < NS; s += RS_NT) {
            const int dy = s / D, o = s - dy * D;
            unsigned s1 = 0, s2 = 0;
            for (int y = 0; y < th; y++) {
                s1 += Hb[(y + dy) * D + o];
                s2 += Hbb[(y + dy) * D + o];
            }
            acc[NS + s] += s1;
            acc[2 * NS + s] += s2;
        }
    }
    if (sa) atomicAdd(&acc[3 * NS], (unsigned long long)sa);
    if (saa) atomicAdd(&acc[3 * NS + 1], (unsigned long long)saa);
    __syncthreads();
    unsigned long long* out = mom + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * (size_t)(3 * NS + 2);
    for (int i = t; i < 3 * NS + 2; i += RS_NT)
        if (acc[i]) atomicAdd(&out[i], acc[i]);
}

// ---- finishing kernel ---------------------------------------------------------------------------------------------
// One block per (label image, cell): the scores of all shifts in f64, then the peak, the refinement and the flags by one
// thread (a scan of at most 33 * 33 scores in the order of the tie rule).
__global__ __launch_bounds__(RS_NT) void rs_finish_kernel(const unsigned long long* __restrict__ mom, MaCellGrid g, int R,
                                                          unsigned ncells, double* __restrict__ res, uint8_t* __restrict__ flags,
                                                          double* __restrict__ table)
{
    __shared__ double sc[(2 * MA_RESIDUAL_MAX_SHIFT + 1) * (2 * MA_RESIDUAL_MAX_SHIFT + 1)];
    const int D = 2 * R + 1, NS = D * D;
    const unsigned long long* m = mom + (size_t)blockIdx.x * (size_t)(3 * NS + 2);
    int oy0, oy1, ox0, ox1;
    rs_domain(g, R, g.cell0 + blockIdx.x % ncells, oy0, oy1, ox0, ox1);
    const long long n = (oy1 > oy0 && ox1 > ox0) ? (long long)(oy1 - oy0) * (long long)(ox1 - ox0) : 0;
    const long long S_a = (long long)m[3 * NS], S_aa = (long long)m[3 * NS + 1];
    const long long va = n * S_aa - S_a * S_a;
    for (int s = threadIdx.x; s < NS; s += RS_NT) {
        const long long S_ab = (long long)m[s], S_b = (long long)m[NS + s], S_bb = (long long)m[2 * NS + s];
        const long long num = n * S_ab - S_a * S_b, vb = n * S_bb - S_b * S_b;
        const double v = (va == 0 || vb == 0) ? NAN : (double)num / (sqrt((double)va) * sqrt((double)vb));
        sc[s] = v;
        if (table) table[(size_t)blockIdx.x * NS + s] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int best = -1, bestd2 = 0;
    for (int s = 0; s < NS; s++) {          // dy ascending, then dx ascending: among equal scores and distances the first stays
        const double v = sc[s];
        if (!ma_finite(v)) continue;
        const int dy = s / D - R, dx = s % D - R, d2 = dx * dx + dy * dy;
        if (best < 0 || v > sc[best] || (v == sc[best] && d2 < bestd2)) { best = s; bestd2 = d2; }
    }
    double* r = res + (size_t)blockIdx.x * 4;
    uint8_t* f = flags + (size_t)blockIdx.x * 2;
    r[3] = sc[R * D + R];
    if (best < 0) {
        r[0] = r[1] = r[2] = NAN;
        f[0] = f[1] = 0;
        return;
    }
    const int py = best / D, px = best % D;
    const double s0 = sc[best];
    auto refine = [&](int pos, int stride) {
        if (pos == 0 || pos == D - 1) return 0.0;
        const double sm = sc[best - stride], sp = sc[best + stride];
        if (!ma_finite(sm) || !ma_finite(sp)) return 0.0;
        const double den = sm - 2.0 * s0 + sp;
        if (!(den < 0.0)) return 0.0;
        const double d = 0.5 * (sm - sp) / den;
        return d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d);
    };
    r[0] = (double)(px - R) + refine(px, 1);
    r[1] = (double)(py - R) + refine(py, D);
    r[2] = s0;
    f[0] = (px == 0 || px == D - 1 || py == 0 || py == D - 1) ? 1 : 0;
    f[1] = 1;
}

} // namespace

extern "C" {

int ma_residual_shift_grid(ma_ctx* ctx, const uint8_t* ref, const uint8_t* b0, const uint8_t* b1, int h, int w, int cell_h,
                           int cell_w, int max_shift,
                           double* shift_x0, double* shift_y0, double* score0_peak, double* score0_zero, uint8_t* at_limit0,
                           uint8_t* valid0, double* table0,
                           double* shift_x1, double* shift_y1, double* score1_peak, double* score1_zero, uint8_t* at_limit1,
                           uint8_t* valid1, double* table1)
{
    MA_REQUIRE(ctx && ref && b0 && shift_x0 && shift_y0 && score0_peak && score0_zero && at_limit0 && valid0, "NULL argument");
    MA_REQUIRE(!b1 || (shift_x1 && shift_y1 && score1_peak && score1_zero && at_limit1 && valid1), "NULL argument");
    MA_REQUIRE(max_shift >= 1 && max_shift <= MA_RESIDUAL_MAX_SHIFT, "max_shift must be in 1 .. 16");
    MaCellGrid g;
    long long ncells;
    MA_TRY(ma_cell_grid(h, w, cell_h, cell_w, &g, &ncells));
    MA_REQUIRE((long long)g.ch * g.cw <= MA_RESIDUAL_MAX_CELL_PIXELS, "a cell must hold at most 2^23 pixels");
    const int R = max_shift;
    const unsigned nimg = b1 ? 2 : 1;
    const bool want_table = table0 || (b1 && table1);
    const RsLds L = rs_lds_layout(R);
    const int NS = L.NS;

    // blocks of a full cell: strips of RS_TW columns, each cut into chunks of tpb tiles of RS_TH rows.  tpb trades global
    // atomics (one flush of the block's accumulators per chunk) against blocks in flight: aim at >= 4096 blocks, at most
    // 16 tiles a block.
    const int nstrip = (g.cw + RS_TW - 1) / RS_TW, ntile = (g.ch + RS_TH - 1) / RS_TH;
    int tpb = 16;
    while (tpb > 1 && (double)ncells * nimg * nstrip * ((ntile + tpb - 1) / tpb) < 4096.0) tpb >>= 1;
    const int nchunk = (ntile + tpb - 1) / tpb;
    // row groups and column segments per quad of shifts: the smallest powers of two that give the block's threads about
    // eight items each
    const int nquad = (2 * R + 1) * ((2 * R + 1 + 3) / 4);
    int G = 1, KS = 1;
    while (G < RS_TH && nquad * G < 8 * RS_NT) G <<= 1;
    while (KS < 4 && nquad * G * KS < 6 * RS_NT) KS <<= 1;

    // per cell and label image: the u64 moments; four doubles, two flags and, if asked for, the table of scores
    const size_t mom_per = (size_t)(3 * NS + 2) * sizeof(unsigned long long);
    const size_t out_per = 4 * sizeof(double) + (want_table ? (size_t)NS * sizeof(double) : 0) + 2;
    long long cap = (long long)(((size_t)64 << 20) / (out_per * nimg));   // page-locked staging stays <= 64 MiB
    if (cap > MA_GRID_Y_MAX) cap = MA_GRID_Y_MAX;
    // results of a batch, on the device and in the page-locked copy: [nblk][4] doubles, the tables, [nblk][2] flags
    const size_t tab_per = want_table ? (size_t)NS : 0;
    return ma_cell_batches(
        ctx, ncells, (mom_per + out_per) * nimg, out_per * nimg, cap,
        [&](long long c0, unsigned nb, const void** dev, size_t* bytes) -> int {
            const size_t nblk = (size_t)nb * nimg;
            unsigned long long* mom = (unsigned long long*)ctx->ws;
            double* res = (double*)(mom + nblk * (size_t)(3 * NS + 2));
            double* tab = res + nblk * 4;
            uint8_t* flags = (uint8_t*)(tab + nblk * tab_per);
            g.cell0 = c0;
            MA_HIP(hipMemsetAsync(mom, 0, nblk * mom_per, ctx->stream));
            {
                MaProfScope ps(ctx, MA_K_OTHER, (double)h * w * nimg * ((double)nb / ncells));
                hipLaunchKernelGGL(rs_corr_kernel, dim3((unsigned)(nstrip * nchunk), nb, nimg), dim3(RS_NT), L.bytes, ctx->stream, ref,
                                   b0, b1, g, L, nchunk, tpb, G, KS, mom);
            }
            hipLaunchKernelGGL(rs_finish_kernel, dim3((unsigned)nblk), dim3(RS_NT), 0, ctx->stream, (const unsigned long long*)mom, g,
                               R, nb, res, flags, want_table ? tab : (double*)nullptr);
            MA_HIP(hipGetLastError());
            *dev = res;
            *bytes = nblk * out_per;
            return MA_OK;
        },
        [&](long long c0, unsigned nb, const void* pinned) {
            const size_t nblk = (size_t)nb * nimg;
            const double* pres = (const double*)pinned;
            const double* ptab = pres + nblk * 4;
            const uint8_t* pfl = (const uint8_t*)(ptab + nblk * tab_per);
            for (unsigned im = 0; im < nimg; im++) {
                double* sx = im ? shift_x1 : shift_x0;
                double* sy = im ? shift_y1 : shift_y0;
                double* sp = im ? score1_peak : score0_peak;
                double* sz = im ? score1_zero : score0_zero;
                uint8_t* al = im ? at_limit1 : at_limit0;
                uint8_t* va = im ? valid1 : valid0;
                double* tb = im ? table1 : table0;
                for (unsigned i = 0; i < nb; i++) {
                    const size_t k = (size_t)im * nb + i;
                    sx[c0 + i] = pres[4 * k];
                    sy[c0 + i] = pres[4 * k + 1];
                    sp[c0 + i] = pres[4 * k + 2];
                    sz[c0 + i] = pres[4 * k + 3];
                    al[c0 + i] = pfl[2 * k];
                    va[c0 + i] = pfl[2 * k + 1];
                    if (tb) memcpy(tb + (size_t)(c0 + i) * NS, ptab + k * NS, (size_t)NS * sizeof(double));
                }
            }
        });
}

} // extern "C"
