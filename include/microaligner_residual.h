/* Residual shift maps: per cell of a regular grid, the translation in pixels that still separates two u8 label images,
 * found by an exhaustive search of the integer shifts within +-max_shift for the largest zero-mean normalised
 * cross-correlation (ZNCC) and refined to sub-pixel by a parabola.  An extension of libmicroaligner_hip.so with no
 * counterpart in the reference; off the measured path (build.source_hash() does not cover it).  It shares no code with the
 * flow solver: it is a check of a registration, not a restatement of it.
 *
 * Cells: the grid of microaligner_qc.h -- from (0, 0), cells of cell_h x cell_w pixels over an (h, w) image,
 * gy = ceil(h / cell_h) rows and gx = ceil(w / cell_w) columns of cells, the last row / column ragged, every output in
 * row-major cell order.
 *
 * Definition, with R = max_shift, a = ref and b = b0 (or b1):
 *   domain   : for the cell [y0, y1) x [x0, x1):  O = [max(y0, R), min(y1, h - R)) x [max(x0, R), min(x1, w - R)), the same
 *              for every shift; a is read on O, b on O + d (up to R px into the neighbouring cells); n = |O|.
 *   moments  : exact integers.  S_a = sum a, S_aa = sum a^2; for every shift d = (dx, dy), |dx|, |dy| <= R:
 *              S_b(d) = sum b(p + d), S_bb(d) = sum b(p + d)^2, S_ab(d) = sum a(p) b(p + d), all sums over p in O;
 *              num = n S_ab - S_a S_b, va = n S_aa - S_a^2, vb = n S_bb - S_b^2  (int64; every product stays below 2^63
 *              because a cell holds at most 2^23 pixels).
 *   score    : score(d) = (double)num / (sqrt((double)va) * sqrt((double)vb)) in IEEE float64, round to nearest, no fused
 *              multiply-add; NaN where va = 0 or vb(d) = 0 (and everywhere when n = 0).
 *   peak     : the largest finite score; ties go to the smallest dx^2 + dy^2, then the smallest dy, then the smallest dx.
 *              A cell without a finite score is invalid: shift_x, shift_y and score are NaN, at_limit is 0.
 *   sub-pixel: per axis, only if the peak is not at +-R on that axis, both neighbours s-, s+ along the axis are finite and
 *              den = s- - 2 s0 + s+ < 0:  delta = 0.5 * (s- - s+) / den clamped to [-0.5, 0.5]; otherwise delta = 0.
 *              shift_x = dx + delta_x, shift_y = dy + delta_y.
 *   sign     : a(p) ~ b(p + shift): the content of b sits `shift` px further along +x / +y than the reference has it.
 *
 * Outputs per cell: shift_x, shift_y, score (at the peak), score_zero (at d = 0), at_limit (the peak lies on the border of
 * the search square: the true shift may be larger, the value is a lower bound), valid, and, where `table` is not NULL, all
 * scores as (gy, gx, 2R + 1, 2R + 1) doubles with dy the slower index (entry [dy + R][dx + R]).
 *
 * Every moment is an integer, so the result does not depend on the order of summation or on the batching: work is done in
 * batches of cells so that the device workspace stays within ma_ctx_set_workspace_limit.  The call synchronises the ctx
 * stream; every output pointer is host memory. */
#ifndef MICROALIGNER_RESIDUAL_H
#define MICROALIGNER_RESIDUAL_H

#include "microaligner_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_RESIDUAL_MAX_SHIFT 16
#define MA_RESIDUAL_MAX_CELL_PIXELS (1 << 23)

/* ref, b0, b1: device pointers to (h, w) u8 labels; b0 and b1 are compared with the same reference in one pass (b1 may be
 * NULL: the second set of outputs is then not written and may be NULL).  table0 / table1 may be NULL.  MA_EINVAL, without
 * touching a device, for a NULL argument, max_shift outside 1 .. 16, h or w < 1, a cell size < 1 or a cell of more than
 * 2^23 pixels. */
int ma_residual_shift_grid(ma_ctx* ctx, const uint8_t* ref, const uint8_t* b0, const uint8_t* b1, int h, int w, int cell_h,
                           int cell_w, int max_shift,
                           double* shift_x0, double* shift_y0, double* score0_peak, double* score0_zero, uint8_t* at_limit0,
                           uint8_t* valid0, double* table0,
                           double* shift_x1, double* shift_y1, double* score1_peak, double* score1_zero, uint8_t* at_limit1,
                           uint8_t* valid1, double* table1);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_RESIDUAL_H */
