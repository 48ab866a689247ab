/* cv2.remap's interpolation modes for the warps of libmicroaligner_hip.so: INTER_NEAREST, INTER_CUBIC and
 * INTER_LANCZOS4 besides the INTER_LINEAR of ma_remap_bilinear / ma_warp_tiled / ma_warp_pages_host.  Off the measured
 * path (build.source_hash() does not cover it).
 *
 * Semantics (OpenCV 4.5.5 imgwarp.cpp, BORDER_CONSTANT 0; unpinned against OpenCV until tests/golden/cv2_remap.npz is
 * recorded):
 *   nearest : each map coordinate is cvRound-ed on its own (round half to even) and saturated to short; the pixel there,
 *             or 0 outside the source.
 *   cubic   : 4 x 4 taps from (sx - 1, sy - 1), lanczos4: 8 x 8 taps from (sx - 3, sy - 3), where sx, sy and the 5-bit
 *             fractions are those of the linear path (cvRound(m * 32)).  1-D weights: interpolateCubic (A = -0.75, float)
 *             and interpolateLanczos4 (sin / cos in double, normalised in float) at x = i / 32; 2-D weights: the float
 *             product vy * vx (u16, f32) or cvRound(vy * vx * 32768) with initInterTab2D's sum fix-up (u8).  A sample whose
 *             taps all lie outside the source is 0.  When every tap lies inside the source the taps of a row are summed
 *             left to right and the row sums in order (lanczos4 from 0); otherwise the taps inside the source are summed
 *             one by one from 0.  u8: (acc + 2^14) >> 15 saturated; u16: cvRound saturated; f32: the float sum.
 * The tiled warp's "source" is the zero-padded window of ma_warp_tiled: a tap in the padding reads 0, a tap beyond the
 * window is skipped.  MA_INTER_LINEAR forwards to the linear entry points and returns their bits. */
#ifndef MICROALIGNER_INTERP_H
#define MICROALIGNER_INTERP_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

enum ma_interp { MA_INTER_NEAREST = 0, MA_INTER_LINEAR = 1, MA_INTER_CUBIC = 2, MA_INTER_LANCZOS4 = 4 };

/* cv2.remap(src, map, None, interp): src (sh, sw, cn) of dtype, map (dh, dw, 2) float32 absolute source coordinates,
 * dst (dh, dw, cn).  cn is 1 to 4 (1 or 2 for MA_INTER_LINEAR, as ma_remap_bilinear).  All dims < 32767. */
int ma_remap_interp(ma_ctx* ctx, const void* src, int dtype, int cn, int sh, int sw, const float* map_xy, int dh, int dw,
                    void* dst, int interp);

/* ma_warp_tiled with the interpolation mode interp. */
int ma_warp_tiled_interp(ma_ctx* ctx, const void* img, int dtype, int H, int W, const float* flow, int tile, int overlap,
                         void* out, int interp);

/* ma_warp_pages_host with the interpolation mode interp: host pages in, host pages out, one device-resident flow,
 * upload, kernel and download overlapped in the bands of ma_warp_pages_plan, by the one page-warp driver that
 * ma_warp_pages_host runs (MICROALIGNER_TRACE_PAGES=1 prints its timeline).  Synchronous. */
int ma_warp_pages_host_interp(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages, int dtype,
                              int H, int W, const float* flow, int tile, int overlap, int interp);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_INTERP_H */
