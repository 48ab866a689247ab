/* Local correlation maps: the Gaussian-windowed zero-mean normalised cross-correlation (ZNCC) of a reference image and
 * another image on the reference's grid (usually the moving image after the warp), per pixel: a dense score in [-1, 1], a
 * weight made from it that the consumers of per-pixel weights take as it is, and per-cell counts of agreeing, disagreeing,
 * flat and unsupported pixels.  They say where the two images agree after the warp: detached tissue, debris, out-of-focus
 * patches and places where a solver locked onto the wrong structure score low.  An extension of libmicroaligner_hip.so with
 * no counterpart in the reference.  Off the measured path (build.source_hash() does not cover it).  Whole image, no tile
 * windows.
 *
 * All arithmetic is float32 and every operation is rounded on its own: nothing is fused, the division and the square root
 * are the correctly rounded ones, denormals are kept, and the arithmetic is IEEE's throughout.
 *
 * Input: ref (H, W) uint8, uint16 or float32 (MA_U8, MA_U16, MA_F32); img (H, W) float32, the other image on the
 *   reference's grid (ma_warp_affine_flow of the float32 moving image, as in ma_flow_refine_step); 1 <= H, W <= 2^24.
 *   Scalars: center_ref, center_img (finite), floor (finite, > 0, in squared grey levels), min_support (finite, >= 0),
 *   lo and hi with -1 <= lo < hi <= 1.
 * Weight, by weight_kind (enum ma_smooth_weight_kind of microaligner_flowsmooth.h; the per-cell kind is refused):
 *   MA_SMOOTH_WEIGHT_NONE: w = 1 (the pointer is ignored); MA_SMOOTH_WEIGHT_F32: an (H, W) float32 map;
 *   MA_SMOOTH_WEIGHT_U8: an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0.
 * Per pixel: A = float32(ref) - center_ref, B = img - center_img.  A pixel is live if w is finite and > 0 and A and B are
 *   finite.  Products of a live pixel, with wa = w * A and wb = w * B:
 *     P0 = w, P1 = wa, P2 = wb, P3 = wa * A, P4 = wb * B, P5 = wa * B;   of any other pixel: six zeros.
 *   The centres exist only for conditioning: the ZNCC does not depend on them mathematically, while in float32 an uncentred
 *   uint16 image loses about a decade of accuracy.
 * Smoothing: taps t[0 .. r] (host, float32), the centre and one side of a symmetric kernel, 1 <= r <= 128, every tap finite
 *   and >= 0, t[0] > 0.  A row pass, then a column pass over the row pass's output, both by the rule of
 *   microaligner_flowsmooth.h along their axis, samples outside the image being 0:
 *     A(x) = t[0] * P(x); then for k = 1 .. r ascending: A = A + t[k] * (P(x - k) + P(x + k)).
 *   The results are Sw, Sa, Sb, Saa, Sbb, Sab (of P0 .. P5).
 * Score: if not (Sw > min_support): s = NaN.  Otherwise
 *     ma = Sa / Sw, mb = Sb / Sw;
 *     va = Saa / Sw - ma * ma, and a negative va becomes 0;  vb = Sbb / Sw - mb * mb, likewise;
 *     c = Sab / Sw - ma * mb;  den = sqrt(va + floor) * sqrt(vb + floor);  s = c / den;
 *     s > 1 becomes 1, s < -1 becomes -1, a NaN stays NaN.
 *   floor is the variance below which a window counts as empty: that of a patch of bare glass.  It makes the score go to 0
 *   on empty windows instead of amplifying noise, and keeps den > 0.
 * Weight out, with span = hi - lo formed once in float32 on the host:
 *     0 if s is NaN or s < lo;  1 if s >= hi;  otherwise (s - lo) / span.
 * Classes, tested in this order: unsupported: s is NaN;  flat: va <= floor and vb <= floor (neither image has content:
 *   not a disagreement);  agree: s >= hi;  disagree: the rest, which includes content in one image and none in the other.
 * Per-cell counts: on the cell grid of microaligner_qc.h (cells of cell_h x cell_w pixels from (0, 0), gy = ceil(H / cell_h)
 *   rows and gx = ceil(W / cell_w) columns of cells, the last row and column ragged; a cell larger than the image is the
 *   whole axis), counts[cy][cx][0 .. 4) = the agreeing, disagreeing, flat and unsupported pixels of the cell, which sum to
 *   its pixel count.  Integer adds: the result does not depend on their order.
 * The sign and payload of a computed NaN are not promised.
 * The zero border of the smoothing lowers Sw within r px of the image's edge, not the score: every sum is divided by Sw. */
#ifndef MICROALIGNER_LOCALCORR_H
#define MICROALIGNER_LOCALCORR_H

#include "microaligner_flowsmooth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_LOCALCORR_MAX_RADIUS 128
#define MA_LOCALCORR_CLASSES 4

/* The maps of ref and img as defined above: a row pass that forms the six products from ref, img and the weight into a
 * 24 B/px workspace from the ctx cache (its planes transposed), then a column pass that ends in the score, the weight and
 * the class counts.  ref, img, weight, score and weight_out ((H, W) float32 each) are device pointers, taps_host and
 * counts_host (gy * gx * 4 entries) host pointers; taps_host is read before the call returns.  Any of score, weight_out and
 * counts_host may be NULL, not all three; only the planes given are written.  cell_h and cell_w are read only when
 * counts_host is given.  Enqueued on the ctx stream; with counts_host == NULL the call only enqueues, otherwise it
 * synchronises the stream.
 * MA_EINVAL, before any device work, for a NULL ctx, ref, img or taps_host, a NULL weight of a kind other than NONE, no
 * output at all, score and weight_out being one array, an unknown dtype, H or W outside [1, 2^24], r outside [1, 128], a tap
 * that is not finite or is negative, t[0] == 0, a centre that is not finite, a floor that is not finite and positive, a
 * min_support that is not finite or is negative, lo and hi not in -1 <= lo < hi <= 1, a weight kind other than NONE, F32 and
 * U8, or a cell size < 1 when it is read. */
int ma_local_correlation(ma_ctx* ctx, const void* ref, int dtype, const float* img, int H, int W, const float* taps_host,
                         int r, float center_ref, float center_img, float floor, const void* weight, int weight_kind,
                         float min_support, float lo, float hi, float* score, float* weight_out, int cell_h, int cell_w,
                         long long* counts_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_LOCALCORR_H */
