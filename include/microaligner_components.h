/* Connected components of an image: labels, the areas and bounding boxes of the components, and the two filters built from
 * them -- remove the objects below a size, fill the enclosed holes up to a size.  They answer what no local filter can:
 * which pixels belong together, which objects are small whatever their shape, which holes are enclosed whatever their
 * size.  An extension of libmicroaligner_hip.so with no counterpart in the reference.  Off the measured path
 * (build.source_hash() does not cover it): nothing in ma_optflow_register calls it.  Whole image, no tile windows.
 *
 * Everything here is integer and defined without a traversal order: two runs give the same bits, whatever order the
 * atomics of the kernels arrive in.
 *
 * 1. Images.  (H, W), single plane, row-major, uint8, uint16 (MA_U8, MA_U16 of microaligner_hip.h) or int32 (MA_CC_I32, the
 *    dtype of the labels this header's own entry writes).  float32 is refused: the caller thresholds first.
 *    1 <= H, W <= 2^24 and H * W <= MA_CC_MAX_PIXELS = 2^31 - 1: the linear index y * W + x of a pixel is an int32.
 *
 * 2. Foreground.  A pixel is foreground when its value is not 0; a negative int32 is foreground.
 *
 * 3. Neighbours.  Without MA_CC_CONN8 the 4 edge neighbours of a pixel, with it the 8 neighbours
 *    (scipy.ndimage.generate_binary_structure(2, 1) and (2, 2)).  Two neighbouring pixels are joined when both are
 *    foreground and, with MA_CC_BY_VALUE, their values are equal.  A component is a class of the transitive closure of that
 *    relation.  With MA_CC_HOLES (ma_cc_filter only) the roles are exchanged: the pixels that are 0 are joined, under the
 *    same neighbours, and MA_CC_BY_VALUE has no meaning and is refused.
 *
 * 4. Numbering.  Component k, k = 1 .. n, is the k-th in ascending order of each component's smallest linear index.
 *    Background is label 0.  Without MA_CC_BY_VALUE that is scipy.ndimage.label(img != 0, structure).
 *
 * 5. Area: the number of pixels of a component.  Box: y0, x0, y1, x1 with the ends exclusive (scipy.ndimage.find_objects as
 *    numbers).  A component touches the border when it has a pixel in row 0, row H - 1, column 0 or column W - 1.
 *
 * How it is computed (csrc/components.hip): a block labels a tile of MA_CC_TILE x MA_CC_TILE pixels in LDS (row runs, then
 * union-find over the runs) and writes every pixel's parent, the linear index of the smallest pixel of its component inside
 * the tile; pairs of neighbours across tile borders are joined in that plane by atomic minima on the roots' words; every
 * pixel's parent is then replaced by its root, which is the component's smallest linear index.  No thread ever waits for
 * another: every loop ends because an integer decreased. */
#ifndef MICROALIGNER_COMPONENTS_H
#define MICROALIGNER_COMPONENTS_H

#include "microaligner_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_CC_I32 3                 /* the dtype code of an int32 image, beside MA_U8, MA_U16 (MA_F32 is refused) */
#define MA_CC_MAX_PIXELS 2147483647 /* H * W at most */
#define MA_CC_TILE 64               /* the side of the tile one block labels in LDS */

enum ma_cc_flags {
    MA_CC_CONN8 = 1,    /* 8 neighbours, not 4 */
    MA_CC_BY_VALUE = 2, /* neighbours are joined only where their values are equal */
    MA_CC_HOLES = 4     /* ma_cc_filter: work on the components of the pixels that are 0 */
};

/* labels[y * W + x] = the number of the pixel's component under flags (MA_CC_CONN8, MA_CC_BY_VALUE), 0 for background;
 * *count = n, the number of components.  src is (H, W) of dtype, labels (H, W) int32, both on the device; labels must not
 * overlap src (the seams are joined by src's values while labels holds the parents).  Workspace from the ctx cache: one
 * int32 plane and one int32 per 1024 pixels, 4 H W + H W / 256 + 8 bytes.  count is a host value, so the call waits for
 * the ctx stream before it returns (six launches and one copy of 4 bytes). */
int ma_cc_label(ma_ctx* ctx, const void* src, int dtype, int H, int W, int flags, int* labels, long long* count);

/* The areas and boxes of a label image: labels is (H, W) int32 on the device with values in 0 .. n (what ma_cc_label wrote,
 * or any image of that kind); areas, n + 1 int64 on the device: areas[k] the number of pixels of value k, areas[0] those of
 * the background; bboxes, (n + 1) x 4 int32 on the device: y0, x0, y1, x1 of value k, zeros for row 0 and for a value no
 * pixel has.  A pixel whose value is outside 0 .. n takes no part.  0 <= n <= 2^31 - 2.  The pixels of one value need not be
 * connected.  A tile adds once per set of pixels of one value that are connected inside it under 8
 * neighbours, so the atomics number the pieces of the components in the tiles, not the pixels.  No workspace.  Enqueued on
 * the ctx stream (three launches); the call does not synchronise. */
int ma_cc_stats(ma_ctx* ctx, const int* labels, int H, int W, long long n, long long* areas, int* bboxes);

/* dst = src with components deleted or filled; src and dst are (H, W) of dtype on the device, dst may be src.  A component
 * is selected when min_area <= its area <= max_area and, with MA_CC_HOLES, it does not touch the border.
 *   without MA_CC_HOLES: the components are those of the foreground (MA_CC_CONN8, MA_CC_BY_VALUE as above); every
 *     foreground pixel of a component that is NOT selected becomes 0; `value` is not used;
 *   with MA_CC_HOLES: the components are those of the pixels that are 0; every pixel of a selected component becomes
 *     `value`, 1 <= value <= the largest value of dtype.
 * Every other pixel comes back bit for bit.  0 <= min_area, max_area <= MA_CC_MAX_PIXELS (max_area < min_area selects
 * nothing).  Workspace from the ctx cache: two int32 planes, 8 H W bytes.  It needs no numbering and no host value: four
 * launches on the ctx stream, no synchronisation. */
int ma_cc_filter(ma_ctx* ctx, const void* src, int dtype, int H, int W, int flags, long long min_area, long long max_area,
                 long long value, void* dst);

/* All three: src, labels, areas, bboxes and dst are device pointers under the alignment rule of microaligner_hip.h ("Device
 * pointers"): each aligned to its element (areas to 8 bytes), and the result is the same bits at any such address (every
 * access is one element wide).  The workspace stays within 12 bytes per pixel (8 at most).
 * MA_EINVAL, before any device work, for a NULL pointer, a dtype that is not MA_U8, MA_U16 or MA_CC_I32, H or W outside
 * [1, 2^24], H * W above MA_CC_MAX_PIXELS, unknown flags, MA_CC_HOLES given to ma_cc_label or together with MA_CC_BY_VALUE,
 * n, min_area or max_area out of range, and a `value` out of range with MA_CC_HOLES. */

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_COMPONENTS_H */
