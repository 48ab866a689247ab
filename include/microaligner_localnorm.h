/* Local contrast normalisation: an image with its Gaussian-windowed local mean taken out and divided by its
 * Gaussian-windowed local standard deviation, per pixel: z = (x - mu) / sqrt(v + floor), clipped, as float32 or as uint8
 * around 128.  A gain and an offset that vary slowly over the image (bleaching, uneven stripping, the illumination of
 * mosaic tiles) leave z unchanged, so two images of one structure come out with one grey level: what Farneback assumes of
 * its inputs.  An extension of libmicroaligner_hip.so with no counterpart in the reference.  Off the measured path
 * (build.source_hash() does not cover it): nothing in ma_optflow_register calls it.  Whole image, no tile windows.
 *
 * All arithmetic is float32 and every operation is rounded on its own: nothing is fused, the division and the square root
 * are the correctly rounded ones, denormals are kept, and the arithmetic is IEEE's throughout.
 *
 * Input: img (H, W) uint8, uint16 or float32 (MA_U8, MA_U16, MA_F32); 1 <= H, W <= 2^24.
 *   Scalars: floor (finite, > 0, in squared grey levels), clip (> 0 and not NaN; +Inf only when no uint8 output is asked
 *   for), min_support (finite, >= 0).
 * Weight, by weight_kind (enum ma_smooth_weight_kind of microaligner_flowsmooth.h; the per-cell kind is refused):
 *   MA_SMOOTH_WEIGHT_NONE: w = 1 (the pointer is ignored); MA_SMOOTH_WEIGHT_F32: an (H, W) float32 map;
 *   MA_SMOOTH_WEIGHT_U8: an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0.
 * Per pixel: x = float32(img).  A pixel is live if w is finite and > 0 and x is finite.
 * Smoothing: taps t[0 .. r] (host, float32), the centre and one side of a symmetric kernel, 1 <= r <= 128, every tap finite
 *   and >= 0, t[0] > 0.  A row pass, then a column pass over the row pass's output, both by the rule of
 *   microaligner_flowsmooth.h along their axis, samples outside the image being 0:
 *     A(x) = t[0] * P(x); then for k = 1 .. r ascending: A = A + t[k] * (P(x - k) + P(x + k)).
 * Stage 1, the local mean: P0 = w and P1 = w * x of a live pixel, two zeros of any other; Sw and Sx are the smoothed P0
 *   and P1.  A pixel is supported if Sw > min_support.  mu = Sx / Sw.
 * Stage 2, the variance about the local mean (not E[x x] - mu mu, which cancels in float32 on uint16 data): of a live and
 *   supported pixel d = x - mu (the pixel's own mu) and P2 = (w * d) * d; of any other pixel P2 = 0.  Sdd is the smoothed
 *   P2, with the same taps.  v = Sdd / Sw;  z = d / sqrt(v + floor).
 *   floor is the variance below which a window counts as empty: that of a patch of bare glass.  It keeps z near 0 on empty
 *   windows instead of amplifying their noise to full contrast, and keeps the root's argument > 0.
 * Outputs, of a live and supported pixel whose z is not NaN:
 *     out_f32 = min(max(z, -clip), clip);
 *     out_u8  = uint8(rint(min(max(z * scale + 128, 0), 255))), the multiply and the add being two rounded operations,
 *               rint rounding halves to even, and scale = 127.0f / clip formed once in float32 by the entry.  Where the
 *               sum is NaN (z = 0 against a scale that overflowed to +Inf) max takes its other operand: 0.
 *   Of every other pixel (dropped, unsupported, or z is NaN: a sum overflowed): +0.0 and 128.  That is "no contrast": no
 *   edge appears at the rim of a mask.
 * Counts, over the whole image: counts[0] dropped: the pixel is not live;  counts[1] unsupported: live, but not supported
 *   or z is NaN;  counts[2] flat: live, supported and v <= floor;  counts[3] clipped: live, supported and |z| > clip.
 *   The first two and the pixels with an output of their own sum to H * W; flat and clipped are properties of supported
 *   pixels and may both hold of one.  Integer adds: the result does not depend on their order.
 * The zero border of the smoothing lowers Sw within r px of the image's edge, not mu or v: every sum is divided by Sw.
 * Invariance: for a gain g > 0 and an offset b, the image g x + b with the floor g g floor has the z of x with floor, up to
 *   rounding; for g a power of two, b = 0 and no overflow or underflow, bit for bit. */
#ifndef MICROALIGNER_LOCALNORM_H
#define MICROALIGNER_LOCALNORM_H

#include "microaligner_flowsmooth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_LOCALNORM_MAX_RADIUS 128
#define MA_LOCALNORM_COUNTS 4

/* The normalised image as defined above, in four launches over a 16 B/px workspace from the ctx cache: a row pass that
 * forms P0 and P1 from the image and the weight (two planes, transposed), a column pass that ends in mu and Sw (two planes,
 * row-major), a row pass that forms P2 from the image, the weight, mu and Sw (into the first plane again), and a column
 * pass that ends in z, the outputs and the counts.  img, weight, out_f32 ((H, W) float32) and out_u8 ((H, W) uint8) are
 * device pointers under the alignment rule of microaligner_hip.h ("Device pointers"): each aligned to its element;
 * taps_host and counts_host (4 entries) are host pointers, and taps_host is read before the call returns.  Either of
 * out_f32 and out_u8 may be NULL, not both; only the planes given are written.  Enqueued on the ctx stream; with
 * counts_host == NULL the call only enqueues, otherwise it synchronises the stream.
 * MA_EINVAL, before any device work, for a NULL ctx, img or taps_host, both outputs NULL, an output that is img, the weight
 * or the other output, an unknown dtype, a weight kind other than NONE, F32 and U8, a NULL weight of a kind other than NONE,
 * H or W outside [1, 2^24], r outside [1, 128], a tap that is not finite or is negative, t[0] == 0, a floor that is not
 * finite and positive, a clip that is NaN or not positive, clip = +Inf with out_u8, a min_support that is not finite or is
 * negative, and an img, float32 weight or out_f32 that is not aligned to its element. */
int ma_normalize_local(ma_ctx* ctx, const void* img, int dtype, int H, int W, const float* taps_host, int r, float floor,
                       float clip, const void* weight, int weight_kind, float min_support, float* out_f32,
                       uint8_t* out_u8, long long* counts_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_LOCALNORM_H */
