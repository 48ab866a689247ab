"""Global translation by exhaustive search: the shift, of tens to thousands of pixels, between two images that are too poor
in corners for the feature stage -- sparse nuclei, an out-of-focus cycle, large smooth tissue.

    tmat, info = align_translation(ref, mov, return_info=True)
    tmat = align_affine(ref, mov, "affine", tmat=tmat)          # the local method takes it from there

Every integer shift of a window is scored by the zero-mean normalised cross-correlation (ZNCC) of the two label images over
that shift's own overlap (include/microaligner_translation.h, csrc/translation.hip): all shifts the overlap allows at the
level of a pyr_down pyramid whose longer side fits `coarse_side`, then a few shifts around twice the peak at every finer
level, and a parabola per axis at the last.  Sign: ref(p) ~ mov(p + shift); the matrix that comes back is
[[1, 0, -shift_x], [0, 1, -shift_y]] in Warper.tmat's convention, so transform_img_with_tmat(mov, shape, tmat) lands on ref.

Translation only: a rotation beyond about a degree, or a scale, lowers the coarse peak.  A periodic sample has several
peaks of one height; info.distinct (the peak less the best score elsewhere, at the coarsest level) says how far the peak
stands out.  Nothing here changes what register() or warp() compute.
"""
import collections
import math

import numpy as np

from ..device import get_context
from ..shared_modules.registration_qc import _check_image, _dog_flags, _labels
from .. import _lib as L


class TranslationLevel(collections.namedtuple("TranslationLevel", "level shape window peak score second n at_limit")):
    """One level of align_translation: the pyramid level (0 = the images), its (h, w), the window searched
    (dx0, dx1, dy0, dy1), the integer peak (dx, dy), its score, the best score more than `exclude` px away, the pixels of the
    overlap at the peak, and whether the peak lies on the window's border."""


class TranslationInfo(collections.namedtuple("TranslationInfo",
                                             "levels shift score score0 distinct at_limit valid accepted")):
    """align_translation(..., return_info=True): a TranslationLevel per level searched, coarsest first; the shift (x, y) in
    px of the images, whether accepted or not; the score of the finest level searched at its peak and at d = 0; distinct,
    the peak less `second` at the coarsest level; at_limit of any level; valid (every level had a finite score); accepted."""


def level_shapes(shape, coarse_side):
    """[(h, w)] of level 0, 1, .. L: L is the first level whose longer side is <= coarse_side, but the pyramid stops before
    the shorter side falls below 32."""
    shapes = [(int(shape[0]), int(shape[1]))]
    while max(shapes[-1]) > coarse_side:
        nxt = ((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2)
        if min(nxt) < 32:
            break
        shapes.append(nxt)
    return shapes


def level_limits(shape, level, max_shift, min_overlap):
    """(X_l, Y_l): the largest |dx|, |dy| searched at a level of this (h, w)."""
    out = []
    for side in (shape[1], shape[0]):
        lim = int(math.floor((1.0 - min_overlap) * side))
        if max_shift is not None:
            lim = min(lim, int(math.ceil(max_shift / 2.0 ** level)))
        out.append(lim)
    return tuple(out)


def level_window(limits, level_peak_above, refine_radius):
    """(dx0, dx1, dy0, dy1) of a level: everything within the limits at the coarsest level (level_peak_above None), else
    refine_radius around twice the peak of the level above, the centre first brought within the limits."""
    win = []
    for axis, lim in enumerate(limits):
        if level_peak_above is None:
            win += [-lim, lim]
        else:
            c = min(max(2 * level_peak_above[axis], -lim), lim)
            win += [max(-lim, c - refine_radius), min(lim, c + refine_radius)]
    return tuple(win)


def search_levels(shapes, search, max_shift, min_overlap, refine_radius, finest_level):
    """The level loop over search(level, window, table) -> the dict of Context.translation_search.
    -> (levels, shift, score, score0, distinct, at_limit, valid)."""
    top = len(shapes) - 1
    last = min(int(finest_level), top)
    levels, peak, res = [], None, None
    distinct, at_limit = float("nan"), False
    for lv in range(top, last - 1, -1):
        window = level_window(level_limits(shapes[lv], lv, max_shift, min_overlap), peak, refine_radius)
        res = search(lv, window, lv == last)
        levels.append(TranslationLevel(lv, shapes[lv], window, (res["dx"], res["dy"]), res["score"], res["second"], res["n"],
                                       res["at_limit"]))
        if not res["valid"]:
            return levels, (0.0, 0.0), float("nan"), float("nan"), distinct, at_limit, False
        if lv == top:
            distinct = res["score"] - res["second"]
        at_limit = at_limit or res["at_limit"]
        peak = (res["dx"], res["dy"])
    dx0, dx1, dy0, dy1 = levels[-1].window
    if dx0 <= 0 <= dx1 and dy0 <= 0 <= dy1:
        score0 = float(res["table"][-dy0, -dx0])
    else:
        score0 = search(last, (0, 0, 0, 0), False)["score"]
    scale = float(2 ** last)
    shift = (scale * (res["dx"] + res["delta_x"]), scale * (res["dy"] + res["delta_y"]))
    return levels, shift, res["score"], score0, distinct, at_limit, True


def finish(found, min_score):
    """-> (tmat, TranslationInfo) of what search_levels found"""
    levels, shift, score, score0, distinct, at_limit, valid = found
    peak_is_zero = valid and levels[-1].peak == (0, 0)
    accepted = bool(valid and (min_score is None or score >= min_score) and (peak_is_zero or score > score0))
    tmat = np.array([[1.0, 0.0, -shift[0]], [0.0, 1.0, -shift[1]]]) if accepted else np.eye(2, 3)
    return tmat, TranslationInfo(levels, shift, score, score0, distinct, bool(at_limit), bool(valid), accepted)


def check_arguments(ref_img, mov_img, labels, max_shift, min_overlap, coarse_side, refine_radius, finest_level, exclude,
                    min_score):
    """Every check of align_translation, without touching a device -> the level shapes."""
    shape = _check_image(ref_img, "ref_img")
    if _check_image(mov_img, "mov_img") != shape:
        raise ValueError(f"ref_img and mov_img differ in shape: {shape} vs {_check_image(mov_img, 'mov_img')}")
    if labels not in ("dog", "u8"):
        raise ValueError(f"labels must be 'dog' or 'u8', got {labels!r}")
    if not isinstance(min_overlap, (int, float, np.integer, np.floating)) or isinstance(min_overlap, bool) or \
            not 0.0 < min_overlap <= 1.0:
        raise ValueError(f"min_overlap must be in (0, 1], got {min_overlap!r}")
    for name, v, lo in (("refine_radius", refine_radius, 1), ("coarse_side", coarse_side, 32), ("finest_level", finest_level, 0),
                        ("exclude", exclude, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
    if max_shift is not None and (isinstance(max_shift, bool) or not isinstance(max_shift, (int, float, np.integer, np.floating))
                                  or not 0 <= max_shift < 1 << 31):
        raise ValueError(f"max_shift must be None or a number >= 0, got {max_shift!r}")
    if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float, np.integer, np.floating))
                                  or min_score != min_score):
        raise ValueError(f"min_score must be None or a number, got {min_score!r}")
    if shape[0] * shape[1] > L.MA_TRANSLATION_MAX_PIXELS:
        raise ValueError(f"an image must hold at most 2^32 pixels, got {shape}")
    shapes = level_shapes(shape, int(coarse_side))
    top = len(shapes) - 1
    X, Y = level_limits(shapes[top], top, max_shift, float(min_overlap))
    if (2 * X + 1) * (2 * Y + 1) > L.MA_TRANSLATION_MAX_SHIFTS:
        raise ValueError(f"the coarsest level, {shapes[top][0]} x {shapes[top][1]}, would search {(2 * X + 1) * (2 * Y + 1)} "
                         f"shifts, more than 2^20: lower coarse_side ({coarse_side}), or give a max_shift or a larger min_overlap")
    if (2 * int(refine_radius) + 1) ** 2 > L.MA_TRANSLATION_MAX_SHIFTS:
        raise ValueError(f"refine_radius {refine_radius} gives more than 2^20 shifts")
    return shapes


def align_translation(ref_img, mov_img, labels="dog", max_shift=None, min_overlap=0.5, coarse_side=512, refine_radius=2,
                      finest_level=0, exclude=2, min_score=None, dog_muladd_fused=False, return_info=False):
    """The 2 x 3 float64 matrix, in Warper.tmat's convention, of the translation that aligns mov_img to ref_img: the ZNCC peak
    over every integer shift, coarse to fine.

    ref_img, mov_img: (H, W) uint8, uint16 or float32, of one shape, numpy or DeviceArray.  labels: "dog" -- the gate's
    labels (sigmas 5 / 9) of every level image, with the rounding model of dog_muladd_fused as assess_registration();
    "u8" -- every level image scaled to uint8 by its minimum and maximum.  max_shift: the largest |shift| per axis in px of
    the images, None for what min_overlap allows.  min_overlap: the share of a side, per axis, that the two images must
    still share at a shift; it bounds the reach to (1 - min_overlap) of the side.  coarse_side: the exhaustive level is the
    first whose longer side is at most this (the pyramid stops before a side falls below 32 px).  refine_radius: the shifts
    searched around twice the peak of the level above, at every finer level.  finest_level: the last level searched; 0 is
    the images themselves, above it the shift is a multiple of 2^finest_level plus the parabola's part.  exclude: the
    Chebyshev distance from the peak within which `second` is not looked for.  min_score: a score below it is not accepted.

    The shift is accepted only if every level had a finite score, the score reaches min_score and, unless the peak is at 0,
    the score is above that of no shift at all; otherwise the identity comes back and info.accepted is False.  Data never
    raises.  return_info: (tmat, TranslationInfo)."""
    shapes = check_arguments(ref_img, mov_img, labels, max_shift, min_overlap, coarse_side, refine_radius, finest_level,
                             exclude, min_score)
    ctx = get_context()
    flags = _dog_flags(dog_muladd_fused)
    refs, movs = [ctx.asdevice(ref_img)], [ctx.asdevice(mov_img)]
    for _ in shapes[1:]:
        refs.append(ctx.pyr_down(refs[-1]))
        movs.append(ctx.pyr_down(movs[-1]))
    made = {}

    def search(level, window, table):
        if level not in made:
            made[level] = (_labels(ctx, refs[level], labels, flags), _labels(ctx, movs[level], labels, flags))
        a, b = made[level]
        return ctx.translation_search(a, b, window, exclude=int(exclude), table=table)

    found = search_levels(shapes, search, max_shift, float(min_overlap), int(refine_radius), int(finest_level))
    tmat, info = finish(found, min_score)
    return (tmat, info) if return_info else tmat


__all__ = ["align_translation", "TranslationInfo", "TranslationLevel"]
