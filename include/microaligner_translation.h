/* Global translation by exhaustive search: the zero-mean normalised cross-correlation (ZNCC) of two u8 label images at
 * every integer shift of a window, each shift over its own overlap of the two images, the peak and a parabolic sub-pixel
 * refinement.  An extension of libmicroaligner_hip.so with no counterpart in the reference; off the measured path
 * (build.source_hash() does not cover it).
 *
 * Definition, with a = ref and b = mov, both (h, w) u8:
 *   sign     : d = (dx, dy) is integer and signed as in microaligner_residual.h: a(p) ~ b(p + d).
 *   domain   : O(d) = { p : p and p + d lie in the image } = rows [max(0, -dy), min(h, h - dy)) x columns
 *              [max(0, -dx), min(w, w - dx));  n(d) = |O(d)|, 0 when |dx| >= w or |dy| >= h.
 *   moments  : exact integers, every sum over p in O(d) and every one a function of d:
 *              S_a = sum a(p), S_aa = sum a(p)^2, S_b = sum b(p + d), S_bb = sum b(p + d)^2, S_ab = sum a(p) b(p + d).
 *   score    : num = n S_ab - S_a S_b, va = n S_aa - S_a^2, vb = n S_bb - S_b^2 as exact integers (they pass 64 bits for
 *              images above 2^23 pixels: 128-bit arithmetic); each is converted to float64 by one round-to-nearest-even of
 *              the exact integer; score(d) = num / (sqrt(va) * sqrt(vb)), four float64 roundings, no fused multiply-add;
 *              NaN where n = 0, va = 0 or vb = 0.  For n <= 2^23 this is the rule of microaligner_residual.h.
 *   peak     : over a window dx0 .. dx1 x dy0 .. dy1, the largest finite score; ties go to the smallest dx^2 + dy^2, then
 *              the smallest dy, then the smallest dx.  Without a finite score the result is invalid.
 *   sub-pixel: per axis, only if the peak is not on the window's border on that axis, both neighbours s-, s+ along the axis
 *              are finite and den = s- - 2 s0 + s+ < 0:  delta = 0.5 * (s- - s+) / den clamped to [-0.5, 0.5]; otherwise 0.
 *   second   : the largest finite score among the shifts more than `exclude` px (Chebyshev distance) from the peak; NaN if
 *              there is none.
 *   at_limit : the peak lies on the border of the window.
 *
 * Every moment is an integer, so nothing depends on the order of summation or on how the work is cut.  The calls that take
 * a ctx synchronise its stream; mom, scores, result and table are host memory. */
#ifndef MICROALIGNER_TRANSLATION_H
#define MICROALIGNER_TRANSLATION_H

#include "microaligner_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_TRANSLATION_MAX_SHIFTS (1 << 20)
#define MA_TRANSLATION_MAX_PIXELS (1LL << 32)

typedef struct ma_translation_result {
    int dx, dy;               /* the peak; 0, 0 when not valid */
    double delta_x, delta_y;  /* the sub-pixel refinement: the shift is (dx + delta_x, dy + delta_y) */
    double score, second;     /* NaN when not valid / when no shift lies beyond `exclude` */
    long long n;              /* n(d) at the peak */
    int at_limit, valid;
} ma_translation_result;

/* ref, mov: device pointers to (h, w) u8 labels.  mom: host, [5][dy1 - dy0 + 1][dx1 - dx0 + 1] in the order S_ab, S_a,
 * S_aa, S_b, S_bb, entry [dy - dy0][dx - dx0].  MA_EINVAL, without touching a device, for a NULL argument, h or w < 1,
 * h * w > 2^32, an empty window or a window of more than 2^20 shifts.  A window may reach beyond +-(w - 1), +-(h - 1):
 * the entries of such shifts are 0. */
int ma_translation_moments(ma_ctx* ctx, const uint8_t* ref, const uint8_t* mov, int h, int w, int dx0, int dx1, int dy0,
                           int dy1, unsigned long long* mom);

/* The scores of a table of moments, [dy1 - dy0 + 1][dx1 - dx0 + 1] doubles.  Host only: no device call, no ctx.  The
 * checks of ma_translation_moments. */
int ma_translation_scores(int h, int w, int dx0, int dx1, int dy0, int dy1, const unsigned long long* mom, double* scores);

/* Moments, scores and the peak rule in one call.  exclude >= 0.  table: NULL, or all scores as for
 * ma_translation_scores. */
int ma_translation_search(ma_ctx* ctx, const uint8_t* ref, const uint8_t* mov, int h, int w, int dx0, int dx1, int dy0,
                          int dy1, int exclude, ma_translation_result* result, double* table);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_TRANSLATION_H */
