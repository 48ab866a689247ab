"""Texture support maps: where an image holds the content that a flow computed on it rests on.

    maps = texture_maps(img, floor=f, cell_size=1000)
    maps.lam_min, maps.lam_max              # (H, W) float32: eigenvalues of the Gaussian-windowed structure tensor
    maps.weight                             # (H, W) float32 in [0, 1): lam_min / (lam_min + floor)
    maps.textured, maps.edges, maps.flat    # (gy, gx) int64: pixels of each class per cell

An extension with no counterpart in the reference (include/microaligner_texture.h, csrc/texture.hip).  The structure tensor
is the G matrix of Lucas-Kanade and Farneback (Shi-Tomasi's measure): where its smaller eigenvalue is large, image content
determines both components of a flow; where only the larger is, there is an edge and only the component across it is
determined (the aperture problem); where both are small -- empty glass -- the solver's window carried over whatever the
nearest tissue gave it.  `weight` feeds smooth_flow, fit_flow_affine, split_flow and local_affine as it is.  Nothing here
changes what register() or warp() compute.
"""
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np

from .. import _lib as L
from ..device import DeviceArray, gaussian_taps, get_context, texture_maps_params
from .registration_qc import _labels, cell_bounds


@dataclass
class TextureMaps:
    """What texture_maps() returns.  The planes are numpy arrays for a numpy image and DeviceArrays for a DeviceArray; the
    per-cell maps are numpy arrays."""
    lam_min: Union[np.ndarray, DeviceArray]             # (H, W) float32: the smaller eigenvalue, in squared grey levels
    lam_max: Union[np.ndarray, DeviceArray]             # (H, W) float32: the larger one
    weight: Union[np.ndarray, DeviceArray, None] = None  # (H, W) float32, with floor: lam_min / (lam_min + floor), 0 for NaN
    cell_bounds: Optional[np.ndarray] = None            # with floor and cell_size: (gy, gx, 4) int64 of (y0, y1, x0, x1)
    textured: Optional[np.ndarray] = None               # (gy, gx) int64: pixels with lam_min > floor
    edges: Optional[np.ndarray] = None                  # (gy, gx) int64: lam_min <= floor < lam_max
    flat: Optional[np.ndarray] = None                   # (gy, gx) int64: the rest, a NaN lam_min included

    def summary(self) -> dict:
        """Shares of the three classes over the whole image (needs floor and cell_size)."""
        if self.textured is None:
            raise ValueError("summary() needs the per-cell counts: give texture_maps() a floor and a cell_size")
        t, e, f = (int(m.sum()) for m in (self.textured, self.edges, self.flat))
        n = t + e + f
        return {"cells": int(self.textured.size), "pixels": n, "textured": t / n, "edges": e / n, "flat": f / n,
                "cells_without_texture": int((self.textured == 0).sum())}


def window_taps(winsize: int) -> np.ndarray:
    """The Gaussian window of the Farneback solver for `winsize` as taps t[0 .. r]: r = winsize // 2, sigma = 0.3 r,
    normalised and rounded to float32 as device.gaussian_taps builds its own.  ValueError unless 1 <= r <= 128."""
    if isinstance(winsize, bool) or not isinstance(winsize, (int, np.integer)) or \
            not 1 <= int(winsize) // 2 <= L.MA_TEXTURE_MAX_RADIUS:
        raise ValueError(f"winsize must be an integer with 1 <= winsize // 2 <= {L.MA_TEXTURE_MAX_RADIUS}, got {winsize!r}")
    r = int(winsize) // 2
    sigma = 0.3 * r
    return gaussian_taps(sigma, (r - 0.5) / sigma)       # ceil(r - 0.5) = r whatever the rounding of the product


def texture_maps(img, sigma: Optional[float] = None, winsize: int = 99, truncate: float = 3.0, labels: Optional[str] = None,
                 floor: Optional[float] = None, cell_size: Union[int, Tuple[int, int], None] = None) -> TextureMaps:
    """The eigenvalues of the structure tensor of an (H, W) uint8, uint16 or float32 image: central-difference gradients,
    their products smoothed by a Gaussian window, lam_min <= lam_max per pixel (include/microaligner_texture.h).

    sigma: None -- the window the flow solver itself uses for `winsize` (r = winsize // 2, sigma = 0.3 r; the default is
    the 99-tap window of register()), so that the maps speak about the support the flow had; otherwise a Gaussian of
    `sigma` px cut at r = max(1, ceil(truncate * sigma)) <= 128, as in smooth_flow.
    labels: None -- the image as it is; "dog" -- the gate's labels first (dog(img, True), sigmas 5 / 9, as in
    assess_registration), so that camera noise does not count as texture.
    floor: in squared grey levels (of the labels, with labels="dog").  With it `weight` = lam_min / (lam_min + floor), which
    is 1/2 where lam_min == floor and 0 where lam_min is 0 or NaN.  Choose it as the lam_min of a region known to be empty
    (the median of maps.lam_min over a patch of bare glass from a first call without floor): pixels no better supported
    than noise then weigh 1/2 or less, tissue close to 1.
    cell_size (an int or (cell_h, cell_w); needs floor): per cell of that grid the number of textured (lam_min > floor),
    edge (lam_min <= floor < lam_max) and flat pixels, with cell_bounds and summary().
    The zero border of the smoothing lowers both eigenvalues within r px of the image's edge.

    numpy in, numpy out; DeviceArray in, DeviceArray out.  Every argument is checked before any device work."""
    if labels is not None and labels != "dog":
        raise ValueError(f"labels must be None or 'dog', got {labels!r}")
    taps = window_taps(winsize) if sigma is None else gaussian_taps(sigma, truncate)
    want = ("lam_min", "lam_max") + (("weight",) if floor is not None else ())
    H, W, _, _, _, _, ch, cw, _ = texture_maps_params(img, taps, floor, cell_size, want)
    ctx = get_context()
    d_img = ctx.asdevice(img)
    if labels == "dog":
        d_img = _labels(ctx, d_img, "dog", 0)
    out = ctx.texture_maps(d_img, taps, floor, cell_size, want)
    planes = {n: (out[n] if isinstance(img, DeviceArray) else out[n].numpy()) for n in want}
    if cell_size is None:
        return TextureMaps(**planes)
    counts = out["counts"]
    return TextureMaps(**planes, cell_bounds=cell_bounds((H, W), (ch, cw)),
                       textured=np.ascontiguousarray(counts[..., 0]), edges=np.ascontiguousarray(counts[..., 1]),
                       flat=np.ascontiguousarray(counts[..., 2]))


__all__ = ["TextureMaps", "texture_maps", "window_taps"]
