/* Changing a flow: a confidence-weighted (normalised) Gaussian smoothing of a dense flow that drops bad pixels, fills them
 * from their surroundings and feathers the result back into the untouched flow, and the per-pixel mask of where a flow
 * folds or is not finite.  An extension of libmicroaligner_hip.so with no counterpart in the reference.  Off the measured
 * path (build.source_hash() does not cover it).  Whole image, no tile windows.
 *
 * All arithmetic is float32 and every operation is rounded on its own: nothing is fused, a division is the correctly
 * rounded one, denormals are kept.  Only det J is float64.
 *
 * 1. Smoothing.  flow and out are (H, W, 2) float32 (u = [..., 0], v = [..., 1]), 1 <= H, W <= 2^24.
 *    taps t[0 .. r] (host, float32): the centre and one side of a symmetric kernel, 1 <= r <= 128, every tap finite and
 *    >= 0, t[0] > 0.
 *    weight, by weight_kind:
 *      MA_SMOOTH_WEIGHT_NONE  : weight(p) = 1 (the pointer is ignored);
 *      MA_SMOOTH_WEIGHT_F32   : an (H, W) float32 map;
 *      MA_SMOOTH_WEIGHT_U8    : an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0;
 *      MA_SMOOTH_WEIGHT_CELLS : a (gy, gx) float32 map on the cell grid of microaligner_qc.h -- cells of cell_h x cell_w
 *                               pixels from (0, 0), gy = ceil(H / cell_h), gx = ceil(W / cell_w), the last row and column
 *                               ragged: weight(x, y) = map[y / cell_h][x / cell_w], looked up per pixel in the kernel and
 *                               never expanded in memory.  cell_h and cell_w are read for this kind only.
 *    Effective weight: w(p) = weight(p) if weight(p) is finite and > 0 and u(p), v(p) are both finite, else w(p) = 0.
 *    Where w = 0, u and v count as 0.  Planes: P0 = w * u, P1 = w * v, P2 = w.
 *    Row pass, then column pass, the same rule along their axis, samples outside the image being 0:
 *      A(x) = t[0] * P(x); then for k = 1 .. r ascending: A = A + t[k] * (P(x - k) + P(x + k)).
 *    The column pass applies the rule to the row pass's output; its results are S0, S1, S2.
 *    Smoothed value: where S2 > min_support, s = (S0 / S2, S1 / S2); elsewhere (a NaN S2 included) s = (NaN, NaN) and the
 *    pixel is counted in `unsupported`, in either mode and whatever the blend then writes.
 *      MA_SMOOTH_ALL   : out = s.
 *      MA_SMOOTH_BLEND : rs(x) = the row rule applied to a row of W ones, cs(y) = the rule applied to a column of H ones;
 *                        sn = cs(y) * rs(x), c = S2 / sn, d = 4 * c - 2, a = d > 0 ? (d < 1 ? d : 1) : 0 (a NaN d gives 0);
 *                        w(p) > 0 and a == 1 : out = flow(p), bit for bit;
 *                        w(p) > 0 and a < 1  : out = s + a * (flow(p) - s), per component;
 *                        w(p) == 0           : out = s.
 *    With weights in {0, 1}, c is the share of the kernel's mass that kept pixels hold: about 1/2 on a straight edge of a
 *    dropped region, so a = 0 there and out is continuous across the edge, and exactly 1 at a pixel with no dropped pixel
 *    within r (Chebyshev distance), which therefore comes back exactly as it was (a == 1 from c >= 3/4 on, so the
 *    rounding of S2 against sn does not matter).  With weights above 1, c saturates; weights below 1 lower c, and the
 *    feathering reads them as partly dropped.
 *    Between weights of very different size the products w * u may overflow; the arithmetic is IEEE's throughout.
 *
 * 2. Fold mask.  bad(p) holds if u(p) or v(p) is not finite, or if det J(p) is finite and <= 0, det J exactly as in
 *    microaligner_qc.h (float64, numpy.gradient derivatives).  keep(p), uint8 (H, W): 0 if some bad q has
 *    |q.x - p.x| <= margin and |q.y - p.y| <= margin, else 1; 0 <= margin <= 32.
 *    counts[0] = folded  : pixels with a finite det J <= 0  (the sum of ma_qc_flow_grid's folded map);
 *    counts[1] = invalid : pixels with a non-finite u or v  (the sum of its invalid map);
 *    counts[2] = dropped : pixels with keep == 0. */
#ifndef MICROALIGNER_FLOWSMOOTH_H
#define MICROALIGNER_FLOWSMOOTH_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

enum ma_smooth_weight_kind { MA_SMOOTH_WEIGHT_NONE = 0, MA_SMOOTH_WEIGHT_F32 = 1, MA_SMOOTH_WEIGHT_U8 = 2, MA_SMOOTH_WEIGHT_CELLS = 3 };
enum ma_smooth_mode { MA_SMOOTH_ALL = 0, MA_SMOOTH_BLEND = 1 };
#define MA_SMOOTH_MAX_RADIUS 128
#define MA_FOLD_MASK_MAX_MARGIN 32

/* out = flow smoothed as defined above: a row pass into a 12 B/px workspace from the ctx cache, then a column pass with the
 * divide and the blend.  flow, weight and out are device pointers, taps_host a host pointer that is read before the call
 * returns; enqueued on the ctx stream.  out may be flow (a thread reads flow for the blend only at the pixel it writes);
 * weight must not be out.  With unsupported_host == NULL the call only enqueues; otherwise it synchronises the stream and
 * writes the count (an integer atomic add per wave: deterministic).  MA_EINVAL for a NULL ctx, flow, taps_host or out, a
 * NULL weight of a kind other than NONE, H or W outside [1, 2^24], r outside [1, 128], a tap that is not finite or is
 * negative, t[0] == 0, an unknown kind or mode, a cell size < 1 for the CELLS kind, or a min_support that is not finite
 * or is negative. */
int ma_smooth_flow(ma_ctx* ctx, const float* flow, int H, int W, const float* taps_host, int r, const void* weight,
                   int weight_kind, int cell_h, int cell_w, int mode, float min_support, float* out,
                   long long* unsupported_host);

/* keep and the three counts of flow as defined above.  flow and keep ((H, W) bytes) are device pointers; enqueued on the
 * ctx stream.  With counts_host == NULL (else 3 entries) the call only enqueues; otherwise it synchronises the stream.
 * MA_EINVAL for a NULL ctx, flow or keep, H or W outside [1, 2^24], or margin outside [0, 32]. */
int ma_flow_fold_mask(ma_ctx* ctx, const float* flow, int H, int W, int margin, unsigned char* keep,
                      long long* counts_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWSMOOTH_H */
