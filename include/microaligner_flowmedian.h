/* Median-filtering a flow: the exact windowed median of each component over a (2r + 1)^2 box, which removes isolated wrong
 * vectors, keeps motion edges and leaves an affine flow untouched, and the per-pixel mask of the vectors that lie far from
 * the median of their surroundings.  An extension of libmicroaligner_hip.so with no counterpart in the reference.  Off the
 * measured path (build.source_hash() does not cover it).  Whole image, no tile windows.
 *
 * A median is an order statistic: the result is one of the input values, bit for bit, whatever the algorithm.  The only
 * float32 arithmetic is the distance d below; each of its operations is rounded on its own, denormals are kept.
 *
 * 1. Inputs.  flow and out are (H, W, 2) float32 (u = [..., 0], v = [..., 1]), 1 <= H, W <= 2^24.  The radius is
 *    1 <= r <= MA_MEDIAN_MAX_RADIUS = 7: windows of 3 x 3 to 15 x 15.
 *    weight, by weight_kind (enum ma_smooth_weight_kind of microaligner_flowsmooth.h), read as a mask only:
 *      MA_SMOOTH_WEIGHT_NONE  : weight(q) = 1 (the pointer is ignored);
 *      MA_SMOOTH_WEIGHT_F32   : an (H, W) float32 map;
 *      MA_SMOOTH_WEIGHT_U8    : an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0;
 *      MA_SMOOTH_WEIGHT_CELLS : a (gy, gx) float32 map on the cell grid of microaligner_qc.h -- cells of cell_h x cell_w
 *                               pixels from (0, 0), gy = ceil(H / cell_h), gx = ceil(W / cell_w), the last row and column
 *                               ragged: weight(x, y) = map[y / cell_h][x / cell_w], looked up per pixel in the kernel and
 *                               never expanded in memory.  cell_h and cell_w are read for this kind only.
 *    Pixel q PARTICIPATES iff weight(q) is finite and > 0 and u(q), v(q) are both finite.
 *
 * 2. Window.  The window of p is the pixels q of the image with |q.x - p.x| <= r and |q.y - p.y| <= r.  There is no
 *    padding: at the border the window is smaller.  n(p) is the number of participating pixels in it, p included if it
 *    participates.
 *
 * 3. Order.  Values are ordered by the order-preserving signed key of a float's bits,
 *      k = (int32) (bits ^ ((bits >> 31) & 0x7fffffff)),  >> the arithmetic shift of the int32 bits,
 *    so that -0.0 < +0.0, denormals stay distinct, and every bit pattern has one key and every key one bit pattern (the
 *    map is its own inverse).  The keys INT32_MIN and INT32_MAX belong to NaNs, never to a finite float.
 *
 * 4. Median.  Per component separately, m_c(p) is the participating value of the window of rank (n - 1) / 2 (integer
 *    division: the lower median) in ascending key order.  With a full window and nothing dropped n is odd and this is the
 *    median.  m is always one of the input values, bit for bit.  With n == 0, m = (NaN, NaN) and the pixel is counted in
 *    `unsupported`.
 *
 * 5. Outliers.  thresh is float32, >= 0, not NaN; +Inf is allowed and means "none".
 *      d(p) = max(|u - m_u|, |v - m_v|), each subtraction a float32 operation (it may overflow to +Inf);
 *      p is an OUTLIER iff it participates and d > thresh;
 *      p is DROPPED iff it does not participate.
 *
 * 6. Outputs.
 *      MA_MEDIAN_ALL      : out(p) = m(p);
 *      MA_MEDIAN_OUTLIERS : outliers and dropped pixels take m(p), every other pixel comes back bit for bit;
 *      keep (optional, (H, W) uint8): 0 for outliers and dropped pixels, else 1, in either mode;
 *      counts[0] = outliers, counts[1] = dropped, counts[2] = unsupported (n == 0; a subset of dropped). */
#ifndef MICROALIGNER_FLOWMEDIAN_H
#define MICROALIGNER_FLOWMEDIAN_H

#include "microaligner_flowsmooth.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

enum ma_median_mode { MA_MEDIAN_ALL = 0, MA_MEDIAN_OUTLIERS = 1 };
enum ma_median_flags { MA_MEDIAN_GENERIC = 1 };   /* force the kernel that serves every radius, also where r <= 3 */
#define MA_MEDIAN_MAX_RADIUS 7

/* out and keep of flow as defined above, in one kernel: a block stages its tile and an r halo as keys and each thread
 * selects both components of its pixels.  Radii 1 to 3 take a kernel that holds the window in registers, unless flags has
 * MA_MEDIAN_GENERIC; both kernels give the same bits.  flow, weight, out and keep are device pointers; enqueued on the ctx
 * stream.  out or keep may be NULL, not both.  NOT in place: a median reads its neighbours, so out must not be flow, and
 * weight must be neither out nor keep.  With counts_host == NULL (else 3 entries) the call only enqueues; otherwise it
 * synchronises the stream and writes the counts (integer atomic adds per wave: deterministic).  MA_EINVAL for a NULL ctx or
 * flow, out and keep both NULL, out == flow, a NULL weight of a kind other than NONE, a weight that is out or keep, H or W
 * outside [1, 2^24], more than 2^31 - 1 tiles of 32 rows x 64 columns (ceil(H / 32) * ceil(W / 64): about 4.4e12 pixels,
 * more than a device holds), r outside [1, 7], an unknown kind or mode, a cell size < 1 for the CELLS kind, a thresh that is NaN or
 * negative, or a bit of flags other than MA_MEDIAN_GENERIC. */
int ma_median_flow(ma_ctx* ctx, const float* flow, int H, int W, int r, const void* weight, int weight_kind, int cell_h,
                   int cell_w, int mode, float thresh, int flags, float* out, unsigned char* keep, long long* counts_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_FLOWMEDIAN_H */
