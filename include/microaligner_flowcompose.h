/* Exact composition of two dense flows: the flow of "warp by first, then warp the result by second".  An extension of
 * libmicroaligner_hip.so with no counterpart in the reference, whose merge_two_flows samples the second flow at the
 * absolute coordinate -first (ma_merge_flows_tiled restates that on purpose).  Off the measured
 * path (build.source_hash() does not cover it).
 *
 * Definition.  With warp(img, f)(p) = img(p - f(p)) (Warper._make_flow_for_remap),
 *   warp(warp(img, first), second)(p) = img(p - second(p) - first(p - second(p))), so
 *   out(p) = second(p) + first sampled at (p - second(p)).
 * first, second and out are (H, W, 2) float32 of one shape, whole image, no tile windows; 1 <= H, W <= 2^24 (pixel
 * coordinates are exact in float32).  Per pixel p = (x, y) with t = second[y, x], every operation a float32 operation
 * rounded on its own (nothing fused):
 *   1. mx = float(x) - t.x, my = float(y) - t.y.
 *   2. cx = fminf(fmaxf(mx, 0), W - 1), cy = fminf(fmaxf(my, 0), H - 1): replicate border, so first is extended, not
 *      zeroed, where the sample leaves the image; a NaN coordinate clamps to 0.
 *   3. cv2.remap's linear sampling without the 16-bit saturation of the integer coordinate: q = cvRound(cx * 32) (half to
 *      even), ix = q >> 5, fx = q & 31, likewise y; second tap index min(ix + 1, W - 1) / min(iy + 1, H - 1); weights
 *      w0 = y0 x0, w1 = y0 x1, w2 = y1 x0, w3 = y1 x1 with x1 = fx / 32, x0 = 1 - x1 (y likewise);
 *      s = v0 w0 + v1 w1 + v2 w2 + v3 w3 summed in that order (top left, top right, bottom left, bottom right), per
 *      component.
 *   4. out = t + s, per component.  A non-finite t therefore yields a non-finite output at that pixel and nowhere else;
 *      a non-finite value of first reaches the outputs whose four taps include it.
 * compose(0, t) == t and compose(m, 0) == m as values. */
#ifndef MICROALIGNER_FLOWCOMPOSE_H
#define MICROALIGNER_FLOWCOMPOSE_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

/* out = compose(first, second) as defined above.  Device pointers, enqueued on the ctx stream.  MA_EINVAL for a NULL
 * argument, H or W outside [1, 2^24], or out == first; out may be second (a thread reads second only at the pixel it
 * writes). */
int ma_compose_flows(ma_ctx* ctx, const float* first, const float* second, int H, int W, float* out);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWCOMPOSE_H */
