/* Flat grey morphology of an image: the running minimum (erosion) and maximum (dilation) over a rectangle, and what is built
 * from the two: opening, closing, white and black top-hat.  They edit the masks that the other tools make and take (shrink a
 * keep mask off a hole's rim, delete specks, close gaps), and the white top-hat removes an uneven additive background and
 * keeps the grey levels of everything narrower than the rectangle.  An extension of libmicroaligner_hip.so with no
 * counterpart in the reference.  Off the measured path (build.source_hash() does not cover it): nothing in
 * ma_optflow_register calls it.  Whole image, no tile windows.
 *
 * A minimum or a maximum is an order statistic: the result is one of the input values, bit for bit, whatever the algorithm.
 * The only arithmetic is the subtraction of the two hats.
 *
 * 1. Images.  src and dst are (H, W) uint8, uint16 or float32 (MA_U8, MA_U16, MA_F32), single plane, row-major,
 *    1 <= H, W <= 2^24.
 *
 * 2. Structuring element.  The flat rectangle of (2 ry + 1) x (2 rx + 1) pixels, 0 <= ry, rx <= MA_MORPH_MAX_RADIUS = 255.
 *    A radius of 0 on an axis leaves that axis alone.
 *
 * 3. Window.  The window of p is the pixels q of the image with |q.x - p.x| <= rx and |q.y - p.y| <= ry.  It is cut at the
 *    border, not padded: at the border the window is smaller.  For integer images that is what a filter with replicated
 *    border pixels gives (scipy.ndimage's mode="nearest").
 *
 * 4. Order.  uint8 and uint16 use the integer order.  float32 uses the order of the signed key of a float's bits,
 *      k = (int32) (bits ^ ((bits >> 31) & 0x7fffffff)),  >> the arithmetic shift of the int32 bits,
 *    the key of microaligner_flowmedian.h: -0.0 < +0.0, denormals stay distinct, -Inf and +Inf are ordinary values.
 *    A NaN -- any pattern with all exponent bits set and a mantissa that is not zero, of either sign -- takes no part in a
 *    window.  A window with no pixel that takes part gives the NaN of bits 0x7fc00000.  Every other result is one of the
 *    input values, bit for bit.  (With ry = rx = 0 a NaN pixel is such a window: it comes back as 0x7fc00000.)
 *
 * 5. Operations.
 *      MA_MORPH_ERODE    : the smallest value of the window that takes part;
 *      MA_MORPH_DILATE   : the largest;
 *      MA_MORPH_OPEN     : DILATE(ERODE(x)), MA_MORPH_CLOSE : ERODE(DILATE(x)), each step being the operation above applied
 *                          to the previous step's result, the NaN rule included;
 *      MA_MORPH_TOPHAT   : x - OPEN(x);
 *      MA_MORPH_BLACKHAT : CLOSE(x) - x.
 *    For the integer types both hats are >= 0 and exact.  For float32 each is one subtraction, rounded once, denormals
 *    kept; where it is NaN (a NaN pixel, an OPEN or CLOSE that is NaN, Inf - Inf) the result is the NaN of bits 0x7fc00000.
 *
 * 6. Identities that hold exactly with these windows: the rectangle is separable (rows, then columns); an erosion of radius
 *    r1 followed by one of radius r2 is the erosion of radius r1 + r2, and likewise for dilations; OPEN <= x <= CLOSE on
 *    the integer types, and OPEN and CLOSE are idempotent. */
#ifndef MICROALIGNER_MORPHOLOGY_H
#define MICROALIGNER_MORPHOLOGY_H

#include "microaligner_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum ma_morph_op {
    MA_MORPH_ERODE = 0,
    MA_MORPH_DILATE = 1,
    MA_MORPH_OPEN = 2,
    MA_MORPH_CLOSE = 3,
    MA_MORPH_TOPHAT = 4,
    MA_MORPH_BLACKHAT = 5
};
#define MA_MORPH_MAX_RADIUS 255

/* dst = op(src) as defined above.  Every ERODE or DILATE is two launches of one kernel -- a pass along x that writes its
 * result transposed, then the same pass over that plane along y, which writes row-major -- so ERODE and DILATE are two
 * launches and the other four are four; the subtraction of a hat is the epilogue of the last one.  The intermediate planes
 * have the dtype of src and come from the ctx cache: one plane (1, 2 or 4 bytes per pixel) for ERODE and DILATE, two planes
 * (2, 4 or 8 bytes per pixel) for the others.  Every plane is written over the whole image by the launch before the one
 * that reads it.  src and dst are device pointers under the alignment rule of microaligner_hip.h ("Device pointers"): each
 * aligned to its element, and the result is the same bits at any such address (a pass reads whole 4-byte words where a
 * line's own address allows it and single elements at its ends).  dst may be src: every op works in place.  Enqueued on
 * the ctx stream; the call does not synchronise.
 * MA_EINVAL, before any device work, for a NULL ctx, src or dst, an unknown dtype or op, H or W outside [1, 2^24], ry or rx
 * outside [0, 255], or more than 2^23 - 1 tiles of 32 lines x 256 pixels in a pass (ceil(H / 32) * ceil(W / 256) and
 * ceil(W / 32) * ceil(H / 256); a tile is a block of 512 threads and a launch holds fewer than 2^32 threads: about 6.9e10
 * pixels). */
int ma_morphology(ma_ctx* ctx, const void* src, int dtype, int H, int W, int op, int ry, int rx, void* dst);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_MORPHOLOGY_H */
