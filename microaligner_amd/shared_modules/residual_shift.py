"""Residual shift maps: how many pixels a registered image is still off, per cell of a regular grid.

    rs = residual_shift(ref_img, mov_img, flow, cell_size=1000, max_shift=4)
    rs.shift_x, rs.shift_y, rs.magnitude     # (gy, gx) float64, px: what is left after the warp
    rs.before.magnitude                      # the same for the unwarped mov_img
    rs.summary()

An extension with no counterpart in the reference, and independent of the flow solver: for every cell the integer shifts
within +-max_shift px are searched for the largest zero-mean normalised cross-correlation of the two label images, and the
peak is refined to sub-pixel by a parabola per axis (include/microaligner_residual.h, csrc/residual_shift.hip).  Sign:
ref(p) ~ img(p + shift), i.e. the content of the judged image sits `shift` px further along +x / +y than the reference has
it.  The labels, the warp, the argument checks and the cell grid are those of assess_registration().  Nothing here changes
what register() or warp() compute.
"""
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

from .. import _lib as L
from ..device import get_context
from .registration_qc import _check_flow, _check_image, _dog_flags, _labels, cell_bounds, cell_size_hw


@dataclass
class ShiftMaps:
    """The maps of one comparison; every map is (gy, gx)."""
    cell_bounds: np.ndarray       # (gy, gx, 4) int64 of (y0, y1, x0, x1)
    max_shift: int
    shift_x: np.ndarray           # float64, px; NaN where not valid
    shift_y: np.ndarray
    score: np.ndarray             # float64: ZNCC at the peak
    score0: np.ndarray            # float64: ZNCC at shift (0, 0)
    at_limit: np.ndarray          # bool: the peak lies on the border of the search square -- the shift is a lower bound
    valid: np.ndarray             # bool: the cell has a comparison domain and a finite score
    table: Optional[np.ndarray] = None    # (gy, gx, 2R + 1, 2R + 1) float64 of all scores, [dy + R, dx + R]

    @property
    def magnitude(self) -> np.ndarray:
        return np.hypot(self.shift_x, self.shift_y)

    def summary(self) -> dict:
        """Median / 95th percentile / max magnitude over the valid cells, the cells at the limit, the worst cell."""
        mag, ok = self.magnitude, self.valid
        out = {"cells": int(ok.size), "cells_valid": int(ok.sum()), "cells_at_limit": int((self.at_limit & ok).sum()),
               "max_shift": int(self.max_shift)}
        if not ok.any():
            out.update({"median": float("nan"), "p95": float("nan"), "max": float("nan"), "worst_cell": None,
                        "worst_cell_bounds": None})
            return out
        worst = np.unravel_index(int(np.argmax(np.where(ok, mag, -1.0))), mag.shape)
        out.update({"median": float(np.median(mag[ok])), "p95": float(np.percentile(mag[ok], 95)), "max": float(mag[worst]),
                    "worst_cell": tuple(int(i) for i in worst),
                    "worst_cell_bounds": tuple(int(v) for v in self.cell_bounds[worst])})
        return out


@dataclass
class ResidualShift(ShiftMaps):
    """residual_shift(): the maps of ref vs the registered image, and in `before` those of ref vs mov_img as given."""
    before: Optional[ShiftMaps] = None

    def summary(self) -> dict:
        out = super().summary()
        if self.before is not None:
            out["before"] = self.before.summary()
        return out


def _check_max_shift(max_shift, shape):
    R = max_shift
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= L.MA_RESIDUAL_MAX_SHIFT:
        raise ValueError(f"max_shift must be an int in 1 .. {L.MA_RESIDUAL_MAX_SHIFT}, got {max_shift!r}")
    if min(shape) <= 2 * R:
        raise ValueError(f"an image of {shape[0]} x {shape[1]} leaves nothing to compare at max_shift {R}: "
                         f"both sides must exceed {2 * R}")
    return int(R)


def residual_shift(ref_img, mov_img, flow, cell_size: Union[int, Tuple[int, int]] = 1000, max_shift: int = 4,
                   labels: str = "dog", warped=None, tile_size: int = 1000, overlap: int = 100, dog_muladd_fused=False,
                   before: bool = True, return_table: bool = False) -> ResidualShift:
    """Per-cell residual translation, in pixels, of mov_img registered onto ref_img by `flow` (what register() returns).

    labels, warped, tile_size, overlap, dog_muladd_fused: as in assess_registration().  flow=None with warped=None compares
    the two images as given (there is then no `before`).  before: also judge the unwarped mov_img, in the same pass.
    return_table: keep all (2 * max_shift + 1)^2 scores of every cell in `.table`."""
    shape = _check_image(ref_img, "ref_img")
    if _check_image(mov_img, "mov_img") != shape:
        raise ValueError(f"ref_img and mov_img differ in shape: {shape} vs {_check_image(mov_img, 'mov_img')}")
    if flow is not None:
        _check_flow(flow, shape)
    if warped is not None and _check_image(warped, "warped") != shape:
        raise ValueError(f"warped must have the images' shape {shape}")
    if labels not in ("dog", "u8"):
        raise ValueError(f"labels must be 'dog' or 'u8', got {labels!r}")
    ch, cw = cell_size_hw(cell_size)
    if min(ch, shape[0]) * min(cw, shape[1]) > L.MA_RESIDUAL_MAX_CELL_PIXELS:
        raise ValueError(f"a cell of {ch} x {cw} holds more than 2^23 pixels")
    R = _check_max_shift(max_shift, shape)
    warps = warped is None and flow is not None
    if warps and (int(tile_size) < 1 or int(overlap) < 0):
        raise ValueError(f"tile_size must be >= 1 and overlap >= 0, got {tile_size}, {overlap}")

    ctx = get_context()
    ref, mov = ctx.asdevice(ref_img), ctx.asdevice(mov_img)
    if warped is not None:
        judged = ctx.asdevice(warped)
    elif flow is not None:
        judged = ctx.warp(mov, ctx.asdevice(flow), int(tile_size), int(overlap))
    else:
        judged = mov
    flags = _dog_flags(dog_muladd_fused)
    l_ref, l_judged = _labels(ctx, ref, labels, flags), _labels(ctx, judged, labels, flags)
    l_mov = _labels(ctx, mov, labels, flags) if before and judged is not mov else None
    after_maps, before_maps = ctx.residual_shift_grid(l_ref, l_judged, l_mov, ch, cw, R, table=bool(return_table))
    bounds = cell_bounds(shape, (ch, cw))
    return ResidualShift(cell_bounds=bounds, max_shift=R, **after_maps,
                         before=ShiftMaps(cell_bounds=bounds, max_shift=R, **before_maps) if before_maps else None)


__all__ = ["ShiftMaps", "ResidualShift", "residual_shift"]
