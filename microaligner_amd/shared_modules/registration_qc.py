"""Registration quality maps: where a registration worked, per cell of a regular grid.

    qc = assess_registration(ref_img, mov_img, flow, cell_size=1000)
    qc.nmi_before, qc.nmi_after      # (gy, gx): the gate's NMI per 2-D cell, before and after the warp
    qc.jac_min, qc.folded            # (gy, gx): where the flow folds the image over itself

An extension with no counterpart in the reference.  Everything runs on the device (include/microaligner_qc.h, csrc/qc.hip):
the labels are the gate's (dog(img, True) through ma_dog_u8) or min-max normalised u8 images, the per-cell NMI is the
gate's score of the cell's pixels (the same doubles ctx.nmi_scores gives for the cropped cell), and the flow statistics
are those of numpy.gradient on the float64 flow.  Nothing here changes what register() or warp() compute.
"""
from dataclasses import dataclass
from typing import Tuple, Union

import numpy as np

from .. import _lib as L
from ..device import DeviceArray, dense_flow, get_context

_IMG_DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32))


def cell_size_hw(cell_size: Union[int, Tuple[int, int]]) -> Tuple[int, int]:
    """int -> (c, c); (cell_h, cell_w) passes.  ValueError for anything below 1."""
    if isinstance(cell_size, (tuple, list)):
        if len(cell_size) != 2:
            raise ValueError(f"cell_size must be an int or (cell_h, cell_w), got {cell_size!r}")
        ch, cw = cell_size
    else:
        ch = cw = cell_size
    for v in (ch, cw):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"cell_size must be >= 1, got {cell_size!r}")
    return int(ch), int(cw)


def cell_bounds(shape: Tuple[int, int], cell_size: Union[int, Tuple[int, int]]) -> np.ndarray:
    """(gy, gx, 4) int64 of (y0, y1, x0, x1): a grid from (0, 0), the last row / column of cells ragged."""
    h, w = int(shape[0]), int(shape[1])
    ch, cw = cell_size_hw(cell_size)
    ys = np.arange(0, h, ch, dtype=np.int64)
    xs = np.arange(0, w, cw, dtype=np.int64)
    out = np.empty((len(ys), len(xs), 4), np.int64)
    out[..., 0] = ys[:, None]
    out[..., 1] = np.minimum(ys + ch, h)[:, None]
    out[..., 2] = xs[None, :]
    out[..., 3] = np.minimum(xs + cw, w)[None, :]
    return out


@dataclass
class FlowQC:
    """Per-cell statistics of a flow (flow_qc()); every map is (gy, gx)."""
    cell_bounds: np.ndarray
    flow_mean: np.ndarray     # float64: mean |flow| over the cell's finite pixels (NaN if none)
    flow_max: np.ndarray      # float32: max |flow| over the cell's finite pixels (NaN if none)
    jac_min: np.ndarray       # float64: min det J over the cell's det-valid pixels (+inf if none)
    folded: np.ndarray        # int64: det-valid pixels with det J <= 0
    invalid: np.ndarray       # int64: pixels with a non-finite flow component

    def summary(self) -> dict:
        return {"cells": int(self.jac_min.size), "folded": int(self.folded.sum()), "invalid": int(self.invalid.sum()),
                "jac_min": float(self.jac_min.min())}


@dataclass
class RegistrationQC(FlowQC):
    """Per-cell similarity before / after the warp and the flow statistics (assess_registration())."""
    nmi_before: np.ndarray = None   # float64: NMI(ref, mov) per cell
    nmi_after: np.ndarray = None    # float64: NMI(ref, warped) per cell
    ncc_before: np.ndarray = None   # float64: Pearson r of the same labels; NaN where either side is constant
    ncc_after: np.ndarray = None

    @property
    def improved(self) -> np.ndarray:
        return self.nmi_after > self.nmi_before

    def summary(self) -> dict:
        out = super().summary()
        gain = self.nmi_after - self.nmi_before
        worst = np.unravel_index(int(np.argmin(gain)), gain.shape)
        out.update({"cells_improved": int(self.improved.sum()), "nmi_before_mean": float(np.mean(self.nmi_before)),
                    "nmi_after_mean": float(np.mean(self.nmi_after)), "worst_cell": tuple(int(i) for i in worst),
                    "worst_cell_gain": float(gain[worst]),
                    "worst_cell_bounds": tuple(int(v) for v in self.cell_bounds[worst])})
        return out


def _check_image(img, name):
    shape, dtype = np.shape(img) if not isinstance(img, DeviceArray) else img.shape, np.dtype(img.dtype)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{name} must be a non-empty 2-D image, got shape {tuple(shape)}")
    if dtype not in _IMG_DTYPES:
        raise ValueError(f"{name} has unsupported dtype {dtype}: uint8, uint16 or float32")
    return tuple(int(s) for s in shape)


def _check_flow(flow, shape):
    fshape = flow.shape if isinstance(flow, DeviceArray) else np.shape(flow)
    if tuple(fshape) != (shape[0], shape[1], 2) or np.dtype(flow.dtype) != np.float32:
        raise ValueError(f"flow must be float32 of shape {(shape[0], shape[1], 2)}, got {np.dtype(flow.dtype)} {tuple(fshape)}")


def _check_cell_pixels(shape, ch, cw):
    if min(ch, shape[0]) * min(cw, shape[1]) >= 1 << 32:
        raise ValueError(f"a cell of {ch} x {cw} holds 2^32 pixels or more")


def _labels(ctx, img, labels, dog_flags):
    if labels == "u8":
        return img if img.dtype == np.uint8 else ctx.normalize_minmax_u8(img)
    if img.dtype != np.float32:
        return ctx.dog_u8(img, 5, 9, flags=dog_flags)
    out, src_max_is_zero = ctx.dog_u8(img, 5, 9, report_zero=True, flags=dog_flags)
    if src_max_is_zero and ctx.minmax(img)[0] < 0:
        raise ValueError("dog labels of a float image whose max is 0 but which is not all zero are not defined on the device")
    return out


def _dog_flags(dog_muladd_fused):
    # OptFlowRegistrator._dog_flags(): True -> both fused forms, an int -> the MA_DOG_* flags themselves
    f = dog_muladd_fused
    return int(f) if isinstance(f, int) and not isinstance(f, bool) else (L.MA_DOG_FUSED_BLUR | L.MA_DOG_FUSED_SCALE if f else 0)


def _flow_maps(ctx, flow, ch, cw):
    jmin, folded, invalid, mean, mx = ctx.qc_flow_grid(flow, ch, cw)
    return dict(flow_mean=mean, flow_max=mx.astype(np.float32), jac_min=jmin, folded=folded, invalid=invalid)


def flow_qc(flow, cell_size: Union[int, Tuple[int, int]] = 1000) -> FlowQC:
    """The flow half of assess_registration(): Jacobian and magnitude statistics per cell, no images.  A FlowGrid is
    expanded on the device first (device.dense_flow)."""
    flow = dense_flow(flow)
    fshape = flow.shape if isinstance(flow, DeviceArray) else np.shape(flow)
    if len(fshape) != 3:
        raise ValueError(f"flow must be float32 of shape (H, W, 2), got shape {tuple(fshape)}")
    shape = (int(fshape[0]), int(fshape[1]))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"flow must be non-empty, got shape {tuple(fshape)}")
    _check_flow(flow, shape)
    ch, cw = cell_size_hw(cell_size)
    ctx = get_context()
    d_flow = ctx.asdevice(flow)
    return FlowQC(cell_bounds=cell_bounds(shape, (ch, cw)), **_flow_maps(ctx, d_flow, ch, cw))


def assess_registration(ref_img, mov_img, flow, cell_size: Union[int, Tuple[int, int]] = 1000, labels: str = "dog",
                        warped=None, tile_size: int = 1000, overlap: int = 100,
                        dog_muladd_fused=False) -> RegistrationQC:
    """Per-cell quality of a registration of mov_img onto ref_img by `flow` (what register() returns).

    labels: "dog" -- the gate's labels (dog(img, True), sigmas 5 / 9, the rounding model dog_muladd_fused selects as on
    OptFlowRegistrator); "u8" -- u8 images as they are, other dtypes min-max normalised to u8.  warped: mov_img already
    warped by `flow`; otherwise it is warped here as Warper(tile_size, overlap) does (register()'s own warp)."""
    shape = _check_image(ref_img, "ref_img")
    if _check_image(mov_img, "mov_img") != shape:
        raise ValueError(f"ref_img and mov_img differ in shape: {shape} vs {_check_image(mov_img, 'mov_img')}")
    _check_flow(flow, shape)
    if warped is not None and _check_image(warped, "warped") != shape:
        raise ValueError(f"warped must have the images' shape {shape}")
    if labels not in ("dog", "u8"):
        raise ValueError(f"labels must be 'dog' or 'u8', got {labels!r}")
    ch, cw = cell_size_hw(cell_size)
    _check_cell_pixels(shape, ch, cw)
    if warped is None and (int(tile_size) < 1 or int(overlap) < 0):
        raise ValueError(f"tile_size must be >= 1 and overlap >= 0, got {tile_size}, {overlap}")

    ctx = get_context()
    ref, mov, d_flow = ctx.asdevice(ref_img), ctx.asdevice(mov_img), ctx.asdevice(flow)
    wrp = ctx.asdevice(warped) if warped is not None else ctx.warp(mov, d_flow, int(tile_size), int(overlap))
    flags = _dog_flags(dog_muladd_fused)
    l_ref, l_mov, l_wrp = (_labels(ctx, a, labels, flags) for a in (ref, mov, wrp))
    nmi_after, nmi_before, ncc_after, ncc_before = ctx.qc_nmi_grid(l_ref, l_wrp, l_mov, ch, cw)
    return RegistrationQC(cell_bounds=cell_bounds(shape, (ch, cw)), **_flow_maps(ctx, d_flow, ch, cw),
                          nmi_before=nmi_before, nmi_after=nmi_after, ncc_before=ncc_before, ncc_after=ncc_after)


__all__ = ["FlowQC", "RegistrationQC", "assess_registration", "flow_qc", "cell_bounds"]
