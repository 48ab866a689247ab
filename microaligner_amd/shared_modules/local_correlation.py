"""Local correlation maps: where two images agree after the warp, per pixel.

    floor = float(np.var(ref[:500, :500].astype(np.float64)))           # a patch of bare glass
    maps = local_correlation(ref, mov, flow, floor=floor, tmat=tmat, cell_size=1000)
    maps.score                                  # (H, W) float32 in [-1, 1]: the Gaussian-windowed ZNCC, NaN = unsupported
    maps.weight                                 # (H, W) float32 in [0, 1]: 0 below lo, 1 from hi on, linear between
    maps.agree, maps.disagree, maps.flat, maps.unsupported      # (gy, gx) int64: pixels of each class per cell

An extension with no counterpart in the reference (include/microaligner_localcorr.h, csrc/local_correlation.hip).  The
weights that existed say where a flow is impossible (fold_mask, flow_qc) or unfounded (texture_maps); this one says where
the images themselves disagree once the flow is applied: tissue that detached between cycles, debris, out-of-focus patches,
places where the solver locked onto the wrong structure.  `weight` feeds smooth_flow, repair_flow, fit_flow_affine,
split_flow, local_affine, align_affine and refine_flow as it is.  Nothing here changes what register() or warp() compute.

The score is blind to gain and bias by construction.  The warp's zero fill outside the moving image reads as disagreement.
The zero border of the smoothing lowers the window's weight within r px of the image's edge, not the score.  The window
dilutes defects smaller than about sigma.
"""
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np

from ..device import DeviceArray, FlowGrid, _check_image, _real, affine_flow_params, dense_flow, gaussian_taps, get_context, \
    local_correlation_params
from .registration_qc import _labels, cell_bounds

_IDENTITY = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
LOCALCORR_WANT = ("score", "weight")


@dataclass
class CorrelationMaps:
    """What local_correlation() returns.  The planes are numpy arrays for a numpy reference image and DeviceArrays for a
    DeviceArray; the per-cell maps are numpy arrays."""
    score: Union[np.ndarray, DeviceArray]          # (H, W) float32 in [-1, 1], NaN where the window has no support
    weight: Union[np.ndarray, DeviceArray]         # (H, W) float32 in [0, 1]: 0 for NaN or < lo, 1 for >= hi
    center: tuple = (0.0, 0.0)                     # the centres that were subtracted, as float32 values
    cell_bounds: Optional[np.ndarray] = None       # with cell_size: (gy, gx, 4) int64 of (y0, y1, x0, x1)
    agree: Optional[np.ndarray] = None             # (gy, gx) int64: pixels with score >= hi
    disagree: Optional[np.ndarray] = None          # (gy, gx) int64: content in either image and score < hi
    flat: Optional[np.ndarray] = None              # (gy, gx) int64: both windowed variances <= floor
    unsupported: Optional[np.ndarray] = None       # (gy, gx) int64: a NaN score

    def summary(self) -> dict:
        """Shares of the four classes over the whole image, and the cell with the largest disagreeing share (needs
        cell_size)."""
        if self.agree is None:
            raise ValueError("summary() needs the per-cell counts: give local_correlation() a cell_size")
        a, d, f, u = (int(m.sum()) for m in (self.agree, self.disagree, self.flat, self.unsupported))
        n = a + d + f + u
        share = self.disagree / (self.agree + self.disagree + self.flat + self.unsupported)
        worst = np.unravel_index(int(np.argmax(share)), share.shape)
        return {"cells": int(self.agree.size), "pixels": n, "agree": a / n, "disagree": d / n, "flat": f / n,
                "unsupported": u / n, "worst_cell": (int(worst[0]), int(worst[1])), "worst_cell_disagree": float(share[worst])}


def _center_arg(center):
    # "median", None, or a pair of finite numbers -> "median" or the pair
    if center is None:
        return (0.0, 0.0)
    if isinstance(center, str):
        if center != "median":
            raise ValueError(f"center must be 'median', None or a pair of numbers, got {center!r}")
        return center
    try:
        ca, cb = center
    except (TypeError, ValueError):
        raise ValueError(f"center must be 'median', None or a pair of numbers, got {center!r}") from None
    ca, cb = _real(ca, "center[0]"), _real(cb, "center[1]")
    if not (np.isfinite(ca) and np.isfinite(cb)):
        raise ValueError(f"the centres must be finite, got {center!r}")
    return (ca, cb)


def _median(ctx, x):
    v = ctx.image_quantiles(x, [0.5])[0][0]
    return float(np.float32(v)) if np.isfinite(v) else 0.0


def local_correlation(ref_img, mov_img, flow=None, *, floor, tmat=None, sigma=4.0, truncate=3.0, weight=None, labels=None,
                      center="median", lo=0.25, hi=0.75, min_support=0.0, cell_size=None) -> CorrelationMaps:
    """The Gaussian-windowed zero-mean normalised cross-correlation of ref_img and the warped mov_img, per pixel
    (include/microaligner_localcorr.h).

    ref_img: (H, W) uint8, uint16 or float32.  With a `flow` ((H, W, 2) float32, or a FlowGrid, which is expanded first) or
    a `tmat` (the 2 x 3 matrix of FeatureRegistrator.register()), mov_img is the ORIGINAL moving image, (h, w) with h <= H
    and w <= W: it is warped once through both, linearly, as refine_flow does.  With neither, mov_img must have ref_img's
    shape and is used as it is: the map before registration, or of an image warped elsewhere.
    floor: required, finite and > 0, in squared grey levels (of the labels, with labels="dog"): the variance below which a
    window counts as empty -- that of a patch of bare glass, np.var(img[:500, :500]).  It makes the score go to 0 on empty
    windows instead of amplifying noise.
    sigma, truncate: the Gaussian window, cut at r = max(1, ceil(truncate * sigma)) <= 128 as in smooth_flow.
    weight: None, an (H, W) float32 map or a uint8 mask; a weight that is NaN or <= 0 drops its pixel from every sum.
    labels: None -- the images as they are; "dog" -- both are replaced by the gate's labels first (dog(img, True), sigmas
    5 / 9, as in assess_registration).
    center: "median" -- the exact median of each image as the kernel sees it (of the labels, of the warped image), rounded
    to float32, 0 for an image without a finite pixel; None -- zeros; (ca, cb) -- given values.  The score does not depend
    on the centres mathematically; in float32 an uncentred uint16 image loses about a decade of accuracy.
    lo, hi: -1 <= lo < hi <= 1; the weight is 0 below lo, 1 from hi on and linear between; hi also divides agree from
    disagree.  The defaults are plain choices, not tuned.  min_support: a pixel whose window holds no more weight than this
    is unsupported (NaN score, weight 0).
    cell_size (an int or (cell_h, cell_w)): per cell of that grid the number of agreeing, disagreeing, flat and unsupported
    pixels, with cell_bounds and summary().

    numpy ref_img in, numpy out; DeviceArray in, DeviceArray out.  Every argument is checked before any device work."""
    if labels is not None and labels != "dog":
        raise ValueError(f"labels must be None or 'dog', got {labels!r}")
    _check_image(ref_img, "ref_img")
    _check_image(mov_img, "mov_img")
    H, W = (int(v) for v in ref_img.shape)
    center = _center_arg(center)
    taps = gaussian_taps(sigma, truncate)
    warp = flow is not None or tmat is not None
    if flow is None:
        flow_shape = (H, W, 2)
    elif isinstance(flow, FlowGrid):
        flow_shape = flow.shape + (2,)
    elif isinstance(flow, (np.ndarray, DeviceArray)) and flow.dtype == np.float32:
        flow_shape = tuple(flow.shape)
    else:
        raise ValueError("flow must be None, an (H, W, 2) float32 numpy array or DeviceArray, or a FlowGrid")
    if flow_shape != (H, W, 2):
        raise ValueError(f"flow must have shape {(H, W, 2)} for a reference image of {(H, W)}, got {flow_shape}")
    if warp:
        tmat = _IDENTITY if tmat is None else tmat
        affine_flow_params(mov_img.shape, np.float32, flow_shape, np.float32, tmat)
    elif tuple(mov_img.shape) != (H, W):
        raise ValueError(f"without a flow or a tmat, mov_img must have ref_img's shape {(H, W)}, got {tuple(mov_img.shape)}")
    stand_in = np.broadcast_to(np.float32(0), (H, W))      # the shape and dtype of what the kernel will get, no data
    _, _, _, _, _, _, _, _, _, _, _, ch, cw, _ = local_correlation_params(
        ref_img, stand_in, taps, floor, (0.0, 0.0) if center == "median" else center, weight, lo, hi, min_support, cell_size,
        LOCALCORR_WANT)

    ctx = get_context()
    ref, mov = ctx.asdevice(ref_img), ctx.asdevice(mov_img)
    if labels == "dog":
        ref, mov = _labels(ctx, ref, "dog", 0), _labels(ctx, mov, "dog", 0)
    mov = ctx.to_f32(mov)
    if warp:
        if flow is None:
            d_flow = ctx.zeros((H, W, 2), np.float32)
        else:
            d_flow = dense_flow(flow) if isinstance(flow, FlowGrid) else ctx.asdevice(flow)
        mov = ctx.warp_affine_flow(mov, d_flow, tmat, "linear")
    if center == "median":
        center = (_median(ctx, ref), _median(ctx, mov))
    weight = None if weight is None else ctx.asdevice(weight)
    out = ctx.local_correlation(ref, mov, taps, floor, center, weight, lo, hi, min_support, cell_size, LOCALCORR_WANT)
    planes = {n: (out[n] if isinstance(ref_img, DeviceArray) else out[n].numpy()) for n in LOCALCORR_WANT}
    center = tuple(float(np.float32(c)) for c in center)
    if cell_size is None:
        return CorrelationMaps(**planes, center=center)
    counts = out["counts"]
    return CorrelationMaps(**planes, center=center, cell_bounds=cell_bounds((H, W), (ch, cw)),
                           agree=np.ascontiguousarray(counts[..., 0]), disagree=np.ascontiguousarray(counts[..., 1]),
                           flat=np.ascontiguousarray(counts[..., 2]), unsupported=np.ascontiguousarray(counts[..., 3]))


__all__ = ["CorrelationMaps", "local_correlation"]
