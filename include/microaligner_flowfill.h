/* Filling a flow across holes of any size: a push-pull fill.  A weighted pyramid of the kept vectors is reduced to 1 x 1
 * (pull) and expanded back (push), kept pixels overriding, so that every pixel comes back finite wherever one vector of the
 * flow was kept, at a cost per pixel that does not depend on the size of the holes.  There is no radius.  An extension of
 * libmicroaligner_hip.so with no counterpart in the reference.  Off the measured path (build.source_hash() does not cover
 * it).  Whole image, no tile windows.
 *
 * Everything is float32.  Every operation below is rounded on its own and nothing is fused; division is correctly rounded;
 * denormals are kept.
 *
 * 0. Inputs.  flow and out are (H, W, 2) float32 (u = [..., 0], v = [..., 1]), 1 <= H, W <= 2^24.
 *    weight, by weight_kind (enum ma_smooth_weight_kind of microaligner_flowsmooth.h):
 *      MA_SMOOTH_WEIGHT_NONE  : weight(p) = 1 (the pointer is ignored);
 *      MA_SMOOTH_WEIGHT_F32   : an (H, W) float32 map;
 *      MA_SMOOTH_WEIGHT_U8    : an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0;
 *      MA_SMOOTH_WEIGHT_CELLS : a (gy, gx) float32 map on the cell grid of microaligner_qc.h -- cells of cell_h x cell_w
 *                               pixels from (0, 0), gy = ceil(H / cell_h), gx = ceil(W / cell_w), the last row and column
 *                               ragged: weight(x, y) = map[y / cell_h][x / cell_w], looked up per pixel in the kernel and
 *                               never expanded in memory.  cell_h and cell_w are read for this kind only.
 *
 * 1. Level 0.  t0(p) = min(weight(p), 1) where weight(p) is finite and > 0 and u(p), v(p) are both finite; otherwise
 *    t0(p) = 0 and p is DROPPED.  a0(p) = f(p) where t0(p) > 0, else (+0, +0): no NaN ever enters a product.  Pixels with
 *    0 < t0 < 1 are BLENDED.  Weights above 1 saturate at 1.
 *
 * 2. Pull.  A level of h x w entries has a parent of ceil(h / 2) x ceil(w / 2).  Levels are pulled until one is 1 x 1:
 *    L levels above level 0 (L = 0 for a flow of one pixel).  Parent (j, i) has the children (2j + dy, 2i + dx), dy, dx in
 *    {0, 1}, written t_dydx, a_dydx; a child outside its level enters as t = 0, a = +0.
 *      sw = (t00 + t01) + (t10 + t11)
 *      s  = (t00 a00 + t01 a01) + (t10 a10 + t11 a11)        per component
 *      a  = s / sw if sw > 0, else +0
 *      t  = min(sw, 1)
 *
 * 3. Top.  G_L = a_L if t_L > 0, else (NaN, NaN).
 *
 * 4. Push, for l = L - 1 down to 0.  The parent image G_{l+1} has hc x wc entries.  Along x the taps of pixel x are
 *      x even: the indices (x / 2 - 1, x / 2)           with the weights (ax, bx) = (0.25, 0.75),
 *      x odd : the indices ((x - 1) / 2, (x + 1) / 2)   with the weights (ax, bx) = (0.75, 0.25),
 *    indices clamped to [0, wc - 1]; the same rule holds along y with (j0, j1), (ay, by) and hc.  Rows first, then columns:
 *      h_j = ax G[j, i0] + bx G[j, i1]      for j = j0, j1
 *      up  = ay h_j0 + by h_j1
 *    and the level's result is
 *      G_l(p) = a_l(p)                       where t_l(p) >= 1, bit for bit,
 *               up                           where t_l(p) == 0,
 *               up + t_l(p) (a_l(p) - up)    otherwise.
 *
 * 5. Output.  out = G_0: a pixel of t0 == 1 comes back bit for bit, whatever lies around it.
 *      counts[0] = dropped     : the pixels with t0 == 0;
 *      counts[1] = blended     : the pixels with 0 < t0 < 1;
 *      counts[2] = unsupported : the output pixels with a non-finite component.  With every pixel dropped that is all of
 *                                them, all NaN; otherwise only sums that overflowed leave any. */
#ifndef MICROALIGNER_FLOWFILL_H
#define MICROALIGNER_FLOWFILL_H

#include "microaligner_flowsmooth.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

/* out of flow as defined above.  The levels 1 to L live in the context's workspace as one 16-byte (a_u, a_v, t, unused)
 * entry per pixel of a level, G written over a in place by the push: with h_0 = H, w_0 = W and h_l = ceil(h_{l-1} / 2),
 * w_l = ceil(w_{l-1} / 2), the call reserves 256 + 16 * sum_{l = 1 .. L} h_l w_l bytes, about 16 H W / 3.  One launch per
 * level and direction: L pulls, then L pushes (one launch for a flow of one pixel).  flow, weight and out are device pointers;
 * enqueued on the ctx stream.  out == flow is allowed: the last push reads its own pixel of the flow and writes the same
 * pixel, and the pulls are finished by then.  weight must not be out.  With counts_host == NULL (else 3 entries) the call
 * only enqueues; otherwise it synchronises the stream and writes the counts (integer atomic adds per wave: deterministic).
 * MA_EINVAL for a NULL ctx, flow or out, a NULL weight of a kind other than NONE, a weight that is out, H or W outside
 * [1, 2^24], more than 2^31 - 1 tiles of 8 rows x 128 columns (ceil(H / 8) * ceil(W / 128)), an unknown kind, or a cell
 * size < 1 for the CELLS kind; the workspace's own error where the levels do not fit the context's limit. */
int ma_fill_flow(ma_ctx* ctx, const float* flow, int H, int W, const void* weight, int weight_kind, int cell_h, int cell_w,
                 float* out, long long* counts_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWFILL_H */
