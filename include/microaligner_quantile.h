/* Robust intensity normalisation: exact order statistics (percentiles) of an image on the device, and the scaling of an
 * image to u8 between two given values.  An extension of libmicroaligner_hip.so with no counterpart in the reference, which
 * scales between the minimum and the maximum (cv2.normalize NORM_MINMAX); off the measured path (build.source_hash() does
 * not cover it).  Every operation below is rounded on its own, nothing is fused.
 *
 * Definition:
 *   population : all n pixels of a u8 / u16 / f32 array.  For f32, NaN and +-Inf are left out and counted (nonfinite), and
 *                -0.0 counts as +0.0 (v + 0.0f).  With the flag MA_Q_IGNORE_ZEROS, pixels equal to 0 are left out and
 *                counted as well (zeros): padded mosaics and sparse nuclei can be more than 99.9 % exact zeros.  pop is the
 *                number of pixels left; pop + nonfinite + zeros = n.
 *   statistic  : for q in [0, 1], rank = (long long) floor(q * (double)(pop - 1)), one float64 product; the value is the
 *                element of that rank, zero-based, of the population sorted ascending (numpy's method="lower").  It is
 *                always a pixel value, so it is defined bit for bit whatever the order of any reduction.  With pop == 0
 *                every value is NaN.
 *   range      : normalize_range_u8(src, lo, hi) is the rule of ma_normalize_minmax_u8 with (lo, hi) in place of
 *                (min, max).  In float64: d = hi - lo, scale = 255 * (d > DBL_EPSILON ? 1 / d : 0), shift = 0 - lo * scale.
 *                Per pixel in float32: v = float(src) * float(scale) + float(shift), a multiply and then an add; then
 *                v = fminf(fmaxf(v, 0), 255), so that a NaN becomes 0 and +Inf and 1e38 become 255; then cvRound (half to
 *                even).  The clamp comes before the rounding: no float to int conversion can overflow.  For lo = min,
 *                hi = max and finite input the result is that of ma_normalize_minmax_u8 (clamping and a monotone rounding
 *                commute).  hi <= lo gives an all-zero image, as a constant image does there.
 *
 * The statistic is found by a most-significant-digit radix select on an order-preserving unsigned key (u8: the value, 8
 * bits; u16: the value, 16 bits; f32: the bits of v + 0.0f with the sign bit flipped for non-negative values and all bits
 * flipped for negative ones), in digits of 8 / 8 + 8 / 11 + 11 + 10 bits: one pass over the image per digit.  Every count
 * is an integer, so two calls give the same bits. */
#ifndef MICROALIGNER_QUANTILE_H
#define MICROALIGNER_QUANTILE_H

#include "microaligner_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_Q_IGNORE_ZEROS 1
#define MA_Q_MAX_RANKS 8
#define MA_Q_MAX_PIXELS (1LL << 40)

/* values[j] = the order statistic q[j] of img (device pointer, n elements, dtype MA_U8 / MA_U16 / MA_F32); 1 <= nq <= 8,
 * q[j] in [0, 1] in any order, repeats allowed.  counts = {pop, nonfinite, zeros}.  values and counts are HOST arrays.
 * Synchronous.  MA_EINVAL, without touching a device, for a NULL argument, n == 0 or n > 2^40, an unknown dtype or flag,
 * nq out of range, a q that is NaN or outside [0, 1]. */
int ma_image_quantiles(ma_ctx* ctx, const void* img, int dtype, size_t n, int flags, const double* q, int nq,
                       double* values, long long counts[3]);
/* dst (n bytes, device) = the range normalisation above.  lo, hi finite.  On the ctx stream.  MA_EINVAL, without touching
 * a device, for a NULL argument, n == 0, an unknown dtype, a lo or hi that is not finite. */
int ma_normalize_range_u8(ma_ctx* ctx, const void* src, int dtype, size_t n, double lo, double hi, uint8_t* dst);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_QUANTILE_H */
