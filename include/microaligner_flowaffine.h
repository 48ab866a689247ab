/* Taking a flow apart: the weighted least-squares moments from which the global (or per-cell) affine part of a dense flow is
 * fitted, and the re-expression of a flow relative to a 2 x 3 matrix.  An extension of libmicroaligner_hip.so with no
 * counterpart in the reference.  Off the measured path (build.source_hash() does not cover it).  Whole image, no tile
 * windows.
 *
 * Conventions: warp(img, f)(p) = img(p - f(p)).  tmat is the 2 x 3 forward matrix of FeatureRegistrator / Warper.tmat:
 * Warper(tmat, f) samples the padded moving image at M (p - f(p)), M = pinv([tmat; 0 0 1]).  For a flow F on an (H, W) grid
 * the sampling position of pixel p = (x, y) is s(p) = p - F(p).  The fit looks for T (2 x 3) minimising
 * sum w(p) |p - T s~(p)|^2, s~ = (s_x, s_y, 1); the residual flow f'(p) = p - T s~(p) then gives M (p - f'(p)) = p - F(p),
 * so Warper(tmat=T, flow=f') samples where Warper(flow=F) does (algebra; the arithmetic rounds).
 *
 * All arithmetic is float64 and every operation is rounded on its own: nothing is fused.  flow is (H, W, 2) float32
 * (u = [..., 0], v = [..., 1]), 1 <= H, W <= 2^24.
 *
 * 1. Moments.  Frame: c = ((W - 1) / 2, (H - 1) / 2).  Per pixel p = (x, y):
 *      X = x - c_x, Y = y - c_y (exact); u, v the flow components widened to float64; a = X - u, b = Y - v.
 *    weight, by weight_kind (enum ma_smooth_weight_kind of microaligner_flowsmooth.h, the same four kinds):
 *      MA_SMOOTH_WEIGHT_NONE  : weight(p) = 1 (the pointer is ignored);
 *      MA_SMOOTH_WEIGHT_F32   : an (H, W) float32 map;
 *      MA_SMOOTH_WEIGHT_U8    : an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0;
 *      MA_SMOOTH_WEIGHT_CELLS : a (gy, gx) float32 map on the cell grid of this call (cell_h, cell_w, below), looked up in
 *                               the kernel and never expanded in memory.
 *    Effective weight, the rule of microaligner_flowsmooth.h: w(p) = weight(p) widened to float64 if weight(p) is finite and
 *    > 0 and u(p), v(p) are both finite, else w(p) = 0.
 *    Trimming, with a prior T0 (6 doubles, row-major 2 x 3, in the centred frame: it maps (a, b) to (X, Y)) and clip > 0:
 *      rho_x = X - ((T0[0] * a + T0[1] * b) + T0[2]),  rho_y = Y - ((T0[3] * a + T0[4] * b) + T0[5]);
 *      the pixel is used only if |rho_x| <= clip and |rho_y| <= clip (a NaN fails).
 *    Every pixel falls in exactly one class, tested in this order:
 *      invalid    : u or v is not finite;
 *      unweighted : w = 0;
 *      trimmed    : a prior is given and the pixel fails its test;
 *      used       : the rest.
 *    Cells: the grid of microaligner_qc.h -- cells of cell_h x cell_w pixels from (0, 0), gy = ceil(H / cell_h),
 *    gx = ceil(W / cell_w), the last row and column ragged, numbered row-major; a cell size above the image's is the whole
 *    axis, so (H, W) is one cell, the whole image.  Per cell, over its used pixels, with wa = w * a and wb = w * b rounded
 *    once, the 14 sums, in this order:
 *      sums[0..5]   : w, wa, wb, wa * a, wa * b, wb * b;
 *      sums[6..11]  : w * X, w * Y, wa * X, wb * X, wa * Y, wb * Y;
 *      sums[12..13] : (w * u) * u, (w * v) * v;
 *    and the four counts, in this order: used, invalid, unweighted, trimmed; they add up to the cell's area.
 *    The terms are defined bit for bit; the order of summation is not, but it is fixed -- per thread in pixel order, the
 *    threads of a tile in a fixed tree, the tiles of a cell in a fixed order and tree, no floating-point atomics -- so two
 *    calls on the same input return the same bits.  Moments are always taken about the global centre c, whatever the cell:
 *    the sums of the cells add up (in exact arithmetic) to the sums of the whole image.
 *
 * 2. Apply.  With A (6 doubles, row-major 2 x 3), in absolute pixel coordinates:
 *      q_x = x - u, q_y = y - v;
 *      out(p) = ( float32(x - ((A[0] * q_x + A[1] * q_y) + A[2])), float32(y - ((A[3] * q_x + A[4] * q_y) + A[5])) ):
 *    the map formula of microaligner_compose.h, subtracted from p.  Non-finite flow values propagate by IEEE's rules.
 *      split : f' = apply(F, T);
 *      join  : F = apply(f', M), the flow that Warper(flow=...) needs to do what Warper(tmat=T, flow=f') does. */
#ifndef MICROALIGNER_FLOWAFFINE_H
#define MICROALIGNER_FLOWAFFINE_H

#include "microaligner_flowsmooth.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

#define MA_FLOW_AFFINE_SUMS 14
#define MA_FLOW_AFFINE_COUNTS 4

/* The sums and counts of section 1 for every cell: sums_host[cell * 14 + k] and counts_host[cell * 4 + k], host arrays of
 * gy * gx cells.  flow and weight are device pointers (flow 8-byte aligned; loaded 16 bytes at a time where it is 16-byte
 * aligned), prior_or_NULL a host pointer to 6 doubles that is read before the call returns; clip is read only with a
 * prior.  The cells go through the device in batches within the ctx's workspace limit; the call synchronises the ctx
 * stream.  MA_EINVAL for a NULL ctx, flow, sums_host or counts_host, a NULL weight of a kind other than NONE, an unknown
 * kind, H or W outside [1, 2^24], a cell size < 1, a flow that is not 8-byte aligned, a prior with a non-finite entry, a
 * clip that is not > 0 (a NaN included) with a prior, or a cell of more than 2^31 - 1 tiles of 510 x 64 pixels. */
int ma_flow_affine_moments(ma_ctx* ctx, const float* flow, int H, int W, const void* weight, int weight_kind, int cell_h,
                           int cell_w, const double* prior_or_NULL, double clip, double* sums_host, long long* counts_host);

/* out = apply(flow, a) of section 2.  flow and out are device pointers, a a host pointer to 6 doubles that is read before
 * the call returns; enqueued on the ctx stream, no synchronisation.  out may be flow (a thread reads flow only at the
 * pixel it writes).  MA_EINVAL for a NULL ctx, flow, a or out, H or W outside [1, 2^24], or a non-finite entry of a. */
int ma_flow_affine_apply(ma_ctx* ctx, const float* flow, int H, int W, const double* a, float* out);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWAFFINE_H */
