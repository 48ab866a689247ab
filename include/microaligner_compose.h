/* One resampling of a moving image through a registration's two stages, the 2 x 3 affine initialisation of
 * FeatureRegistrator and the flow of OptFlowRegistrator, instead of transform_img_with_tmat followed by Warper.warp().
 * Off the measured path (build.source_hash() does not cover it).
 *
 * Definition.  img (h, w) of dtype u8 / u16 / f32, flow (H, W, 2) float32 with h <= H and w <= W, M the 3 x 3 matrix
 * pinv([T; 0 0 1]) in float64 of the 2 x 3 transform_matrix T (rows 0-1 of it are the m[6] below, row-major), and
 * (pad_left, pad_top) the padding pad_to_shape(img, (H, W)) applies.  For every output pixel p = (x, y) with
 * (fx, fy) = flow[y, x]:
 *   qx = x - fx, qy = y - fy                              (float64)
 *   mx = float32((m[0] * qx + m[1] * qy) + m[2])          (every operation rounded in float64, none fused)
 *   my = float32((m[3] * qx + m[4] * qy) + m[5])
 *   out[p] = cv2.remap(pad_to_shape(img, (H, W)), (mx, my), interp) with BORDER_CONSTANT 0,
 * in the arithmetic of include/microaligner_interp.h (u8 15-bit tables with the sum fix-up, the straight-or-border
 * summation order of cubic and Lanczos-4).  The padded image is never built: a tap reads img at (sx - pad_left,
 * sy - pad_top), 0 outside it.  One deliberate difference to cv2.remap: integer source coordinates are not saturated to
 * 16 bits, so sides of 32767 px and more work; for smaller sides the result is cv2.remap's.  A non-finite or huge map
 * coordinate (NaN / Inf / 1e12 in the flow) rounds to INT_MIN and the sample reads 0.
 *
 * Whole image: no tile windows (Warper.tile_size / overlap do not apply).  With the identity and no padding the result
 * is ma_remap_interp(img, grid - flow), not the tiled output of ma_warp_tiled, which zeroes samples beyond a window.  It
 * is not bit-identical to the two-stage output either: that one interpolates twice (and truncates integer pages to the
 * input dtype in between).
 *
 * Invalid arguments (unknown interp, h > H or w > W, a padding that does not fit, a non-finite m) return MA_EINVAL. */
#ifndef MICROALIGNER_COMPOSE_H
#define MICROALIGNER_COMPOSE_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

/* out (H, W) = one resampling of img (h, w) at float32(M.(p - flow(p))); m = rows 0-1 of M, row-major.  Device
 * pointers, enqueued on the ctx stream; interp: MA_INTER_NEAREST / _LINEAR / _CUBIC / _LANCZOS4. */
int ma_warp_affine_flow(ma_ctx* ctx, const void* img, int dtype, int h, int w, int pad_left, int pad_top,
                        const float* flow, int H, int W, const double m[6], void* out, int interp);

/* the same for host pages (h, w) -> host pages (H, W), one device-resident flow: page i + 1 is uploaded whole while page i
 * is warped, the output leaves in bands of MA_OPT_WARP_BAND_BYTES so that its download overlaps the kernel: the one
 * page-warp driver that ma_warp_pages_host runs, with a single upload piece per page (MICROALIGNER_TRACE_PAGES=1 prints
 * its timeline).  Synchronous. */
int ma_warp_affine_flow_pages_host(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages,
                                   int dtype, int h, int w, int pad_left, int pad_top, const float* flow, int H, int W,
                                   const double m[6], int interp);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_COMPOSE_H */
