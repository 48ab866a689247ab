/* Grid flows: a flow kept as its values on a coarse grid of nodes, one node every s pixels, and bilinear interpolation
 * between them -- 1/s^2 of the dense flow's size -- with everything a stored registration is used for evaluated straight
 * from the nodes: the expansion, the loss against the dense flow per cell, the one-resampling warp of
 * microaligner_compose.h and the point transforms of microaligner_flowinvert.h.  An extension of libmicroaligner_hip.so
 * with no counterpart in the reference.  Off the measured path (build.source_hash() does not cover it).
 *
 * Every operation below is rounded on its own (nothing fused); divisions are correctly rounded.
 *
 * Axis.  n >= 1 pixels, integer stride s >= 1:
 *   g(n, s) = 1 if n == 1, else ceil((n - 1) / s) + 1 nodes, at the pixel positions P_k = min(k * s, n - 1):
 *   the last interval may be shorter than s and is never empty.  A stride above n - 1 gives the two end nodes.
 *   Pixel x lies in cell i = min(x / s, g - 2) (integer division) with weight
 *     t = float32(x - P_i) / float32(P_{i+1} - P_i);
 *   with g == 1: i = 0, t = 0 and the "next" node is node 0 again.
 *
 * Grid.  nodes is (gh, gw, 2) float32, gh = g(H, s), gw = g(W, s), of a flow of shape (H, W, 2).
 *
 * Sample.  nodes[j, i] = flow[Py_j, Px_i]: point sampling.
 *
 * Expand.  With n00, n01 (row j: columns i, i + 1) and n10, n11 (row j + 1) the nodes of the pixel's cell, per
 * component, in float32:
 *   E(x, y) = (n00 * (1 - tx) + n01 * tx) * (1 - ty) + (n10 * (1 - tx) + n11 * tx) * ty.
 * For finite nodes E gives the nodes back at their positions, and with s = 1 the flow itself.  A non-finite node reaches
 * exactly the pixels of the cells it is a corner of (0 * Inf = NaN included).
 *
 * Loss.  Per pixel e = max(fabsf(E.x - f.x), fabsf(E.y - f.y)) in float32; if either difference is NaN the pixel counts
 * as invalid and is left out.  Per cell of the cell grid of microaligner_qc.h (cell_h x cell_w pixels from (0, 0), the
 * last row and column ragged, a cell size above the image is the image): max_err, the float32 maximum of e (NaN when the
 * cell has no valid pixel), above, the number of valid pixels with e > tol, and invalid.  A maximum and two integer
 * counts: none depends on the order of the reduction.
 *
 * Warp.  ma_warp_affine_grid is ma_warp_affine_flow (microaligner_compose.h) with flow(p) = E(p), bit for bit, in all
 * four interpolation modes and the three dtypes; the dense flow is never built.  Whole image, no tile windows.
 *
 * Points.  ma_transform_points_grid is ma_transform_points (microaligner_flowinvert.h) with the sampler S64 replaced by
 *   G64(mx, my): cx = fmin(fmax(mx, 0), W - 1) (a NaN clamps to 0), i = min(floor(cx) / s, gw - 2),
 *     tx = (cx - P_i) / (P_{i+1} - P_i) in float64 (i = 0, tx = 0 with gw == 1), likewise y; the nodes converted to
 *     double, and the expression of E evaluated in float64.
 *   MA_POINTS_TO_MOVING, MA_POINTS_TO_REFERENCE, converged and inside are as defined there.  In real arithmetic G64
 *   equals S64 of the expanded flow (bilinear interpolation of samples of a function that is bilinear on each cell, the
 *   cell borders at integer positions); the two differ by the float32 roundings of E.
 *
 * Limits: 1 <= H, W <= 2^24 (2^30 for the warp), s >= 1 (a stride above max(H, W) means the same as max(H, W)).
 * Invalid arguments return MA_EINVAL. */
#ifndef MICROALIGNER_FLOWGRID_H
#define MICROALIGNER_FLOWGRID_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

/* nodes (gh, gw, 2) = the samples of flow (H, W, 2) at the node positions.  Device pointers, on the ctx stream. */
int ma_flow_grid_sample(ma_ctx* ctx, const float* flow, int H, int W, int s, float* nodes);

/* out (H, W, 2) = E of nodes (gh, gw, 2).  Device pointers, on the ctx stream. */
int ma_flow_grid_expand(ma_ctx* ctx, const float* nodes, int H, int W, int s, float* out);

/* The loss maps of (flow, nodes) per cell of cell_h x cell_w pixels: max_err, above and invalid are HOST arrays of
 * gy x gx = ceil(H / cell_h) x ceil(W / cell_w) entries, row-major.  flow and nodes are device pointers.  Synchronous.
 * tol must not be NaN. */
int ma_flow_grid_error(ma_ctx* ctx, const float* flow, const float* nodes, int H, int W, int s, int cell_h, int cell_w,
                       float tol, float* max_err, long long* above, long long* invalid);

/* ma_warp_affine_flow with the flow given by its nodes (gh, gw, 2) at stride s. */
int ma_warp_affine_grid(ma_ctx* ctx, const void* img, int dtype, int h, int w, int pad_left, int pad_top,
                        const float* nodes, int H, int W, int s, const double m[6], void* out, int interp);

/* ma_warp_affine_flow_pages_host with the flow given by its device-resident nodes: the same page-warp driver and the same
 * band plan (MA_OPT_WARP_BAND_BYTES); a band may start and end inside a grid cell.  Synchronous. */
int ma_warp_affine_grid_pages_host(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages,
                                   int dtype, int h, int w, int pad_left, int pad_top, const float* nodes, int H, int W,
                                   int s, const double m[6], int interp);

/* ma_transform_points with the flow given by its nodes (gh, gw, 2) at stride s; every other argument as there. */
int ma_transform_points_grid(ma_ctx* ctx, const double* pts, int n, const float* nodes, int H, int W, int s,
                             const double* m6, const double* t6, int pad_left, int pad_top, int direction, int max_iter,
                             double tol, double* out, unsigned char* converged, unsigned char* inside);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWGRID_H */
