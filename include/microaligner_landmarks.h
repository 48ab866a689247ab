/* Flows from landmark pairs: a thin-plate spline (TPS) fitted on the host and evaluated on the device, densely, on the
 * nodes of a grid flow (microaligner_flowgrid.h), or at points.  An extension of libmicroaligner_hip.so with no counterpart
 * in the reference.  Off the measured path (build.source_hash() does not cover it).  Convention as in
 * microaligner_flowcompose.h: warp(img, f)(p) = img(p - f(p)).
 *
 * A pair (r_i, m_i), both (x, y) in pixels as float64, says that the reference-frame point r_i shows what the ORIGINAL
 * moving image shows at m_i.  The spline is the sampling map s(p) = p - f(p) with s(r_i) = m_i (smoothing == 0) or close
 * to it (smoothing > 0).
 *
 * 1. Fit (host, numpy float64; microaligner_amd/optflow_reg/landmarks.py).  n landmarks, 3 <= n <= 4096.
 *      c = mean(r), k = 1 / sqrt(mean |r - c|^2), u_i = (r_i - c) * k               normalised centres
 *      K_ij = U(|u_i - u_j|^2), U(q) = 0.5 * q * log(q), U(0) = 0                   (= rho^2 log rho, rho = sqrt(q))
 *      P = [u_i, 1]                                                                 (n, 3)
 *      lambda_n = smoothing * k^2, smoothing >= 0 in px^2
 *      solve [[K + lambda_n I, P], [P^T, 0]] [w; a] = [m; 0]                        w (n, 2), a (3, 2)
 *    Refused: arrays that are not (n, 2) and equal in shape, non-finite values, n outside [3, 4096], a negative or
 *    non-finite smoothing, and, in this order:
 *      (1) collinear landmarks: the 2 x 2 covariance of u has det <= 1e-12 * trace^2;
 *      (2) two exactly equal reference points when smoothing == 0;
 *      (3) a singular system;
 *      (4) a fit that fails the self-check max_i |m_i - s(r_i) - lambda_n w_i| > 1e-6 px (s evaluated as in 2. on the
 *          host): a condition, not a tolerance.
 *    With these definitions the fit is scipy.interpolate.RBFInterpolator(kernel="thin_plate_spline", degree=1,
 *    smoothing=smoothing) on the unnormalised landmarks.
 *
 * 2. Evaluation (device) at a position (x, y) given as doubles.  cw holds n records (u.x, u.y, w.x, w.y); a6 = (a00, a01,
 *    a02, a10, a11, a12) is the affine part in normalised coordinates, row 0 for s.x.  Every operation is a float64
 *    operation rounded on its own (nothing fused); log is the device library's double logarithm.
 *      X = (x - c_x) * k, Y = (y - c_y) * k; Sx = Sy = 0
 *      for i = 0 .. n - 1 in ascending order, one chain per position:
 *        d = X - u_i.x, e = Y - u_i.y, q = d * d + e * e
 *        U = q > 0 ? (0.5 * q) * log(q) : 0
 *        Sx = Sx + w_i.x * U, Sy = Sy + w_i.y * U
 *      s.x = ((a00 * X + a01 * Y) + a02) + Sx, s.y = ((a10 * X + a11 * Y) + a12) + Sy
 *    The single ascending chain makes the three outputs below agree bit for bit where they evaluate the same position.
 *
 * 3. Outputs.
 *      flow: node (j, i) of the grid of an (H, W) flow at `stride` sits at pixel (x, y) = (min(i * stride, W - 1),
 *        min(j * stride, H - 1)), the node positions of microaligner_flowgrid.h, and holds
 *        (float32(x - s.x), float32(y - s.y)).  g(n, s) = 1 for n == 1, else ceil((n - 1) / s) + 1 nodes per axis;
 *        stride == 1 is the dense flow.
 *      points: out = s itself in float64; a non-finite point gives (NaN, NaN).
 *
 * MA_LANDMARK_CHUNK: the number of landmarks the kernels take per step of the landmark loop.  1: the loop is not chunked;
 * every wave reads one 32-byte record per step with wave-uniform (scalar) loads. */
#ifndef MICROALIGNER_LANDMARKS_H
#define MICROALIGNER_LANDMARKS_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

#define MA_LANDMARK_CHUNK 1
#define MA_LANDMARK_MAX 1048576 /* 2^20 records per call */

/* out ((g(H, stride), g(W, stride), 2) float32, device) = the flow of the spline on the nodes of the grid, as defined
 * above, one kernel launch enqueued on the ctx stream.  cw: n x 4 doubles on the device, 32-byte aligned; a6: 6 doubles on
 * the host.  n == 0 evaluates the affine part alone (cw is not read, but must not be NULL).  MA_EINVAL for a NULL ctx, cw,
 * a6 or out, n outside [0, 2^20], H or W outside [1, 2^24], stride < 1, or a non-finite a6, cx, cy or k. */
int ma_landmark_flow(ma_ctx* ctx, const double* cw, int n, const double* a6, double cx, double cy, double k, int H, int W,
                     int stride, float* out);

/* out ((m, 2) float64, device) = s at the m points pts ((m, 2) float64, device), one thread per point, enqueued on the ctx
 * stream; out may be pts (a thread reads only the point it writes).  MA_EINVAL for a NULL pointer, n outside [0, 2^20],
 * m < 0, or a non-finite a6, cx, cy or k. */
int ma_landmark_points(ma_ctx* ctx, const double* cw, int n, const double* a6, double cx, double cy, double k,
                       const double* pts, int m, double* out);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_LANDMARKS_H */
