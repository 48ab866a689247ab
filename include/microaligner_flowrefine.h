/* Refining a flow against the images: one regularised Lucas-Kanade step.  Given the reference image, the moving image
 * already warped by the flow, and the flow, the step solves per pixel the 2 x 2 system of the Gaussian-windowed structure
 * tensor of the warped image (the matrix of microaligner_texture.h) plus `floor` on its diagonal against the windowed
 * gradient-residual products, and adds the solution to the flow.  Where the image has structure the update follows it;
 * where it has none the floor makes the update vanish.  An extension of libmicroaligner_hip.so with no counterpart in the
 * reference.  Off the measured path (build.source_hash() does not cover it).  Whole image, no tile windows.
 *
 * All arithmetic is float32 and every operation is rounded on its own: nothing is fused, a division is the correctly
 * rounded one, denormals are kept, and the arithmetic is IEEE's throughout.
 *
 * Input: ref (H, W) uint8, uint16 or float32 (MA_U8, MA_U16, MA_F32), R = float32(ref); warped (H, W) float32, Wp: the
 *   moving image resampled by the flow (ma_warp_affine_flow of the float32 moving image, linear); flow (H, W, 2) float32
 *   (u = [..., 0], v = [..., 1]); 1 <= H, W <= 2^24.
 * Gradients of Wp, central differences with a replicated border (the rule of microaligner_texture.h):
 *   gx(x, y) = 0.5f * (Wp(min(x + 1, W - 1), y) - Wp(max(x - 1, 0), y)),
 *   gy(x, y) = 0.5f * (Wp(x, min(y + 1, H - 1)) - Wp(x, max(y - 1, 0)));   e = Wp - R.
 * Weight, by weight_kind (enum ma_smooth_weight_kind of microaligner_flowsmooth.h; the per-cell kind is refused):
 *   MA_SMOOTH_WEIGHT_NONE: w = 1 (the pointer is ignored); MA_SMOOTH_WEIGHT_F32: an (H, W) float32 map;
 *   MA_SMOOTH_WEIGHT_U8: an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0.
 * A pixel is live if w is finite and > 0 and Wp, R, gx and gy are all finite.  Products of a live pixel, with
 *   a = w * gx and b = w * gy:  P0 = a * gx, P1 = a * gy, P2 = b * gy, P3 = a * e, P4 = b * e;  of any other pixel: five
 *   zeros.
 * Smoothing: taps t[0 .. r] (host, float32), the centre and one side of a symmetric kernel, 1 <= r <= 128, every tap finite
 *   and >= 0, t[0] > 0.  A row pass, then a column pass over the row pass's output, both by the rule of
 *   microaligner_flowsmooth.h along their axis, samples outside the image being 0:
 *     A(x) = t[0] * P(x); then for k = 1 .. r ascending: A = A + t[k] * (P(x - k) + P(x + k)).
 *   The results are Sxx, Sxy, Syy, Sxe, Sye (of P0 .. P4).
 * Solve, with floor finite and > 0 (in squared grey levels, the floor of ma_texture_maps for the same image and window):
 *   a = Sxx + floor, c = Syy + floor, det = a * c - Sxy * Sxy;
 *   dx = (c * Sxe - Sxy * Sye) / det, dy = (a * Sye - Sxy * Sxe) / det.
 *   If det is not finite or not > 0, or dx or dy is not finite: dx = dy = 0, and the pixel counts as invalid.
 *   Clamp, with max_step finite and > 0: a component > max_step becomes max_step, one < -max_step becomes -max_step; a
 *   pixel where either component was changed counts as clamped.
 *   out = (u + dx, v + dy): a non-finite u or v stays non-finite, the step of such a pixel is counted like any other.
 *   Sign: the warp reads the moving image at p - flow(p), so the warped image after the step is about
 *   Wp(p - d) ~ Wp - g.d, which the system sets to R in the least-squares sense over the window.
 * Statistics of a step, independent of the order of the adds: stats[0] = invalid and stats[1] = clamped (pixel counts);
 *   stats[2] = the bit pattern, as an integer, of step_max: the largest |dx| or |dy| after the clamp over all pixels (0 for
 *   an invalid pixel), taken as an unsigned maximum over the bit patterns of these non-negative floats.
 * The zero border of the smoothing lowers the tensor within r px of the image's edge while floor stays: steps shrink there. */
#ifndef MICROALIGNER_FLOWREFINE_H
#define MICROALIGNER_FLOWREFINE_H

#include "microaligner_flowsmooth.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

#define MA_REFINE_MAX_RADIUS 128
#define MA_REFINE_STATS 3

/* out = flow + one step as defined above: a row pass that forms the five products from ref, warped and the weight into a
 * 20 B/px workspace from the ctx cache (its planes transposed), then a column pass that ends in the solve, the clamp and the
 * add.  ref, warped, weight, flow and out are device pointers, taps_host and stats_host (MA_REFINE_STATS entries) host
 * pointers; taps_host is read before the call returns.  out may be flow (a thread reads flow only at the pixel it writes);
 * ref, warped and weight must not be out.  Enqueued on the ctx stream; with stats_host == NULL the call only enqueues,
 * otherwise it synchronises the stream.
 * MA_EINVAL, before any device work, for a NULL ctx, ref, warped, taps_host, flow or out, a NULL weight of a kind other than
 * NONE, an unknown dtype, H or W outside [1, 2^24], r outside [1, 128], a tap that is not finite or is negative, t[0] == 0, a
 * floor or max_step that is not finite and positive, a weight kind other than NONE, F32 and U8, or out being ref, warped or
 * weight. */
int ma_flow_refine_step(ma_ctx* ctx, const void* ref, int dtype, const float* warped, int H, int W, const float* taps_host,
                        int r, float floor, const void* weight, int weight_kind, float max_step, const float* flow,
                        float* out, long long* stats_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWREFINE_H */
