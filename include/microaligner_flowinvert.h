/* Coordinates through a registration: the dense inverse of a flow, and points mapped between the registered frame (the
 * flow's grid, where the reference lives) and the moving frame (the original moving image).  An extension of
 * libmicroaligner_hip.so with no counterpart in the reference.  Off the measured path (build.source_hash() does not
 * cover it).  Convention as in microaligner_flowcompose.h: warp(img, f)(p) = img(p - f(p)).  Whole image, no tile windows.
 *
 * 1. Dense inverse.  flow f and out g are (H, W, 2) float32, 1 <= H, W <= 2^24.  g satisfies g(q) = -f(q - g(q)), so
 *    compose(f, g) ~ 0: warping by f and then by g gives the image back.  Per pixel q = (x, y), every operation a float32
 *    operation rounded on its own (nothing fused):
 *      sampler S(f; mx, my):
 *        cx = fminf(fmaxf(mx, 0), W - 1), cy = fminf(fmaxf(my, 0), H - 1): replicate border, a NaN clamps to 0;
 *        x0 = floorf(cx), ax = cx - x0, ix = (int)x0, ix1 = min(ix + 1, W - 1); likewise y;
 *        per component, v00 = f[iy, ix], v01 = f[iy, ix1], v10 = f[iy1, ix], v11 = f[iy1, ix1]:
 *        top = v00 * (1 - ax) + v01 * ax, bot = v10 * (1 - ax) + v11 * ax, s = top * (1 - ay) + bot * ay.
 *        Unlike microaligner_flowcompose.h the coordinate is NOT quantised to 1/32 px: with that sampler the iteration
 *        falls into limit cycles between two quantisation cells.
 *      iteration: g = (0, 0); for k = 1 .. max_iter:
 *        n = -S(f; float(x) - g.x, float(y) - g.y); dx = |n.x - g.x|, dy = |n.y - g.y|; g = n;
 *        stop when dx <= tol && dy <= tol (a NaN never stops the loop).
 *      out = g; residual (optional, (H, W) float32) = max(dx, dy) of the last step taken, NaN if either is NaN;
 *      not_converged = the number of pixels that took all max_iter steps without stopping.
 *    A pixel's iterates depend on no other pixel's.  A non-finite value of f reaches the pixels whose iterates sample it
 *    and no others.  The iteration converges where f is a contraction (the adjacent differences of a component along x
 *    and along y sum to less than 1 px per px); where f folds it does not, and not_converged / residual say where.
 *
 * 2. Points.  pts and out are (n, 2) float64 as (x, y), 0 <= n < 2^31.  S64 is the sampler above in float64: the taps
 *    are converted to double, every operation rounded on its own.  M = rows 0-1 of pinv([T; 0 0 1]) and (pad_left,
 *    pad_top) are those of microaligner_compose.h, T the 2 x 3 transform_matrix; a NULL matrix is the identity.
 *      MA_POINTS_TO_MOVING (registered -> moving), p a point of pts:
 *        u = p - S64(f; p.x, p.y);
 *        out.x = ((M[0] * u.x + M[1] * u.y) + M[2]) - pad_left, out.y = ((M[3] * u.x + M[4] * u.y) + M[5]) - pad_top:
 *        the coordinate ma_warp_affine_flow samples at, kept in float64.  converged = 1.
 *      MA_POINTS_TO_REFERENCE (moving -> registered), s a point of pts:
 *        a.x = (T[0] * (s.x + pad_left) + T[1] * (s.y + pad_top)) + T[2], a.y likewise with T[3 .. 5];
 *        solve p - f(p) = a: p = a; for k = 1 .. max_iter: n = a + S64(f; p.x, p.y); dx = |n.x - p.x|, dy = |n.y - p.y|;
 *        p = n; stop when dx <= tol && dy <= tol.  out = p; converged = 1 if the loop stopped, 0 after max_iter steps.
 *      inside = 1 if the registered-frame coordinate (p of pts for TO_MOVING, the final p for TO_REFERENCE) lies in
 *      [0, W - 1] x [0, H - 1] before clamping, else 0.
 *      A non-finite input point gives out = (NaN, NaN), converged = 0 and inside = 0. */
#ifndef MICROALIGNER_FLOWINVERT_H
#define MICROALIGNER_FLOWINVERT_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

enum ma_points_direction { MA_POINTS_TO_MOVING = 0, MA_POINTS_TO_REFERENCE = 1 };

/* out = the inverse of flow as defined above, one kernel launch.  Device pointers, on the ctx stream; residual may be
 * NULL.  With not_converged_host == NULL the call only enqueues; otherwise it synchronises the stream and writes the
 * count (an integer atomic add per wave: deterministic).  MA_EINVAL for a NULL ctx, flow or out, H or W outside
 * [1, 2^24], max_iter < 1, a negative or non-finite tol, or out == flow. */
int ma_invert_flow(ma_ctx* ctx, const float* flow, int H, int W, int max_iter, float tol, float* out, float* residual,
                   long long* not_converged_host);

/* out, converged (n bytes) and inside (n bytes) of the n points pts in `direction`, as defined above, one thread per
 * point.  pts, flow, out, converged and inside are device pointers; m6 (used by TO_MOVING) and t6 (used by TO_REFERENCE)
 * are host pointers to 6 doubles or NULL for the identity.  Enqueued on the ctx stream.  MA_EINVAL for a NULL pointer
 * other than m6 / t6, n < 0, H or W outside [1, 2^24], a non-finite matrix, an unknown direction, max_iter < 1, or a
 * negative or non-finite tol; out may be pts (a thread reads only the point it writes). */
int ma_transform_points(ma_ctx* ctx, const double* pts, int n, const float* flow, int H, int W, const double* m6,
                        const double* t6, int pad_left, int pad_top, int direction, int max_iter, double tol, double* out,
                        unsigned char* converged, unsigned char* inside);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWINVERT_H */
