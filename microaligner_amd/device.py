"""Device context, HBM-resident arrays and the primitive operations of the hot path.

Thin Python over the C-ABI (include/microaligner_hip.h).  One `Context` per HIP
device per process; `DeviceArray` is a dense row-major array in HBM.  All work is
stream ordered on the context's stream, so intermediate results never visit the host.
"""
import collections
import ctypes as C
import os
import threading
import weakref
import zlib

import numpy as np

from . import _lib as L

_DT = {np.dtype(np.uint8): L.MA_U8, np.dtype(np.uint16): L.MA_U16, np.dtype(np.float32): L.MA_F32}


def _dt(dtype):
    dtype = np.dtype(dtype)
    if dtype not in _DT:
        raise ValueError(f"unsupported image dtype {dtype}: the HIP path handles uint8, uint16 and float32")
    return _DT[dtype]


INTERPOLATIONS = {"nearest": L.MA_INTER_NEAREST, "linear": L.MA_INTER_LINEAR, "cubic": L.MA_INTER_CUBIC,
                  "lanczos4": L.MA_INTER_LANCZOS4}


def interp_code(mode):
    """cv2's interpolation code of a mode given by name ("nearest", "linear", "cubic", "lanczos4") or by that code
    (0, 1, 2, 4); ValueError for anything else."""
    if isinstance(mode, str) and mode in INTERPOLATIONS:
        return INTERPOLATIONS[mode]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and int(mode) in INTERPOLATIONS.values():
        return int(mode)
    raise ValueError(f"unknown interpolation {mode!r}: expected one of {sorted(INTERPOLATIONS)} or cv2's codes 0, 1, 2, 4")


def affine_flow_params(img_shape, img_dtype, flow_shape, flow_dtype, tmat, interpolation="linear"):
    """Checks and host-side arguments of the one-resampling warp through a 2x3 matrix and a flow
    (include/microaligner_compose.h), without touching a device: (interp code, rows 0-1 of M = pinv([tmat; 0 0 1]) as 6
    float64 -- formed as transform_img_with_tmat forms it --, pad_left, pad_top of pad_to_shape(img, flow's (H, W))).
    ValueError for an unknown mode or dtype, a tmat that is not a finite 2x3 matrix, or an image larger than the flow."""
    interp = interp_code(interpolation)
    _dt(img_dtype)
    if len(img_shape) != 2:
        raise ValueError(f"expected a 2D grayscale image, got shape {tuple(img_shape)}")
    if len(flow_shape) != 3 or flow_shape[2] != 2 or np.dtype(flow_dtype) != np.float32:
        raise ValueError(f"flow must be (H, W, 2) float32, got {np.dtype(flow_dtype)} {tuple(flow_shape)}")
    try:
        t = np.asarray(tmat, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"tmat must be a finite 2x3 matrix: {e}") from None
    if t.shape != (2, 3) or not np.all(np.isfinite(t)):
        raise ValueError(f"tmat must be a finite 2x3 matrix, got shape {t.shape}")
    (h, w), (H, W) = img_shape, flow_shape[:2]
    if h < 1 or w < 1 or h > H or w > W:
        raise ValueError(f"the image {(h, w)} must be non-empty and no larger than the flow {(H, W)} in either dimension")
    m = np.linalg.pinv(np.append(t, [[0, 0, 1]], axis=0))[:2].ravel()
    return interp, m, (W - w) // 2, (H - h) // 2


POINT_DIRECTIONS = {"to_moving": L.MA_POINTS_TO_MOVING, "to_reference": L.MA_POINTS_TO_REFERENCE}


def _check_flow(flow, name="flow"):
    if getattr(flow, "dtype", None) != np.float32 or len(flow.shape) != 3 or flow.shape[2] != 2:
        raise ValueError(f"{name} must be an (H, W, 2) float32 flow")
    H, W = flow.shape[:2]
    if not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
        raise ValueError(f"flow sides must be in [1, 2^24], got {(H, W)}")
    return int(H), int(W)


def _check_iteration(max_iter, tol, tol_dtype):
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or not 1 <= int(max_iter) < 1 << 31:
        raise ValueError(f"max_iter must be an integer in [1, 2^31), got {max_iter!r}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)):
        raise ValueError(f"tol must be a number, got {tol!r}")
    with np.errstate(over="ignore"):
        t = tol_dtype(tol)
    if not (np.isfinite(t) and t >= 0):
        raise ValueError(f"tol must be finite and not negative as {np.dtype(tol_dtype)}, got {tol!r}")
    return int(max_iter), float(t)


def invert_flow_params(flow, max_iter, tol):
    """Checks of the dense flow inverse (include/microaligner_flowinvert.h) without touching a device:
    (H, W, max_iter, tol as the float32 the kernel compares with).  ValueError for anything the C entry would refuse."""
    H, W = _check_flow(flow)
    return (H, W) + _check_iteration(max_iter, tol, np.float32)


def transform_points_params(points, flow, direction, tmat, image_shape, max_iter, tol):
    """Checks and host-side arguments of the point transforms (include/microaligner_flowinvert.h) without touching a
    device: (points as a C-contiguous (N, 2) float64 array, direction code, the 6 doubles of the matrix that direction
    uses or None, pad_left, pad_top, max_iter, tol).  tmat and image_shape are Warper.tmat and the shape of the moving
    image it resamples (default: the flow's (H, W)); the matrix and the padding come from affine_flow_params.
    `flow` may be a FlowGrid.  ValueError for anything else."""
    if isinstance(flow, FlowGrid):
        H, W = flow.shape
        if H > 1 << 24 or W > 1 << 24:
            raise ValueError(f"flow sides must be in [1, 2^24], got {(H, W)}")
        flow_shape, flow_dtype = (H, W, 2), np.float32
    else:
        H, W = _check_flow(flow)
        flow_shape, flow_dtype = flow.shape, flow.dtype
    if not isinstance(direction, str) or direction not in POINT_DIRECTIONS:
        raise ValueError(f"unknown direction {direction!r}: expected one of {sorted(POINT_DIRECTIONS)}")
    if not isinstance(points, np.ndarray) or points.dtype != np.float64 or points.ndim != 2 or points.shape[1] != 2:
        raise ValueError("points must be an (N, 2) float64 numpy array of (x, y)")
    if points.shape[0] >= 1 << 31:
        raise ValueError("at most 2^31 - 1 points per call")
    max_iter, tol = _check_iteration(max_iter, tol, np.float64)
    mat, left, top = None, 0, 0
    if tmat is None:
        if image_shape is not None:
            raise ValueError("image_shape only has a meaning together with tmat")
    else:
        try:
            shape = (H, W) if image_shape is None else tuple(int(v) for v in image_shape)
        except (TypeError, ValueError):
            raise ValueError(f"image_shape must be (h, w), got {image_shape!r}") from None
        _, m, left, top = affine_flow_params(shape, np.float32, flow_shape, flow_dtype, tmat)
        mat = m if direction == "to_moving" else np.asarray(tmat, np.float64).ravel()
    return np.ascontiguousarray(points), POINT_DIRECTIONS[direction], mat, left, top, max_iter, tol


# ---- smoothing a flow, fold mask (include/microaligner_flowsmooth.h) -------------------------------------------------------
SMOOTH_MODES = {"all": L.MA_SMOOTH_ALL, "blend": L.MA_SMOOTH_BLEND}


def _real(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number, got {v!r}")
    return float(v)


def _finite_f32(v, name):
    x = _real(v, name)
    with np.errstate(over="ignore"):
        x = np.float32(x)
    if not np.isfinite(x):
        raise ValueError(f"{name} must be finite as float32, got {v!r}")
    return float(x)


def _positive_f32(v, name):
    x = _finite_f32(v, name)
    if not x > 0:
        raise ValueError(f"{name} must be finite and positive as float32, got {v!r}")
    return x


def _matrix_2x3(m, name):
    """a finite 2 x 3 matrix as 6 float64 in row order"""
    try:
        t = np.array(m, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a 2 x 3 matrix") from None
    if t.shape != (2, 3) or not np.all(np.isfinite(t)):
        raise ValueError(f"{name} must be a finite 2 x 3 matrix")
    return np.ascontiguousarray(t).ravel()


def _image_sides(H, W):
    if not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
        raise ValueError(f"image sides must be in [1, 2^24], got {(H, W)}")


def _check_taps(taps):
    if not isinstance(taps, np.ndarray) or taps.dtype != np.float32 or taps.ndim != 1:
        raise ValueError("taps must be a 1-D float32 numpy array t[0 .. r]")
    r = taps.shape[0] - 1
    if not 1 <= r <= L.MA_SMOOTH_MAX_RADIUS:
        raise ValueError(f"r must be in [1, {L.MA_SMOOTH_MAX_RADIUS}], got {r}")
    if not (np.all(np.isfinite(taps)) and np.all(taps >= 0) and taps[0] > 0):
        raise ValueError("taps must be finite and not negative, the centre tap positive")
    return np.ascontiguousarray(taps), int(r)


def gaussian_taps(sigma, truncate=3.0):
    """The taps t[0 .. r] of smooth_flow(): r = max(1, ceil(truncate * sigma)), t_k = exp(-k^2 / (2 sigma^2)) in float64,
    divided by t_0 + 2 sum(t_k), then rounded to float32.  ValueError for a sigma or truncate that is not finite and
    positive, or r > 128."""
    sigma, truncate = _real(sigma, "sigma"), _real(truncate, "truncate")
    if not (np.isfinite(sigma) and sigma > 0 and np.isfinite(truncate) and truncate > 0):
        raise ValueError(f"sigma and truncate must be finite and positive, got {sigma!r}, {truncate!r}")
    rr = np.ceil(truncate * sigma)
    if not rr <= L.MA_SMOOTH_MAX_RADIUS:
        raise ValueError(f"r = ceil(truncate * sigma) = {rr:.0f} exceeds {L.MA_SMOOTH_MAX_RADIUS}: smooth in rounds, or lower "
                         "truncate")
    k = np.arange(max(1, int(rr)) + 1, dtype=np.float64)
    t = np.exp(-k * k / (2.0 * sigma ** 2))
    return (t / (t[0] + 2.0 * t[1:].sum())).astype(np.float32)


def _cell_size_hw(cell_size):
    try:
        ch, cw = (cell_size, cell_size) if isinstance(cell_size, (int, np.integer)) else cell_size
        ok = all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 1 <= int(v) < 1 << 31 for v in (ch, cw))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"cell_size must be a positive integer or a pair of them, got {cell_size!r}")
    return int(ch), int(cw)


def _weight_kind(weight, H, W, cell_size=None, cells=None):
    """(kind, cell_h, cell_w) of a weight argument: None, or an (H, W) float32 or uint8 array (numpy or device), or a per-cell
    map as far as `cells` says the call takes one:
      None    never (direct_affine_moments, flow_refine_step, local_correlation); cell_size is not theirs to pass;
      "map"   with cell_size a (gy, gx) float32 map on that cell grid and nothing else; cell_size has no meaning without
              one (smooth_flow, median_flow, fill_flow);
      "grid"  cell_size is the grid of the call whatever the weight, None standing for one cell, and the weight is per
              pixel or a float32 map of the grid's shape (flow_affine_moments).
    cell_h, cell_w: the cells, (H, W) for the one cell of "grid", else (1, 1)."""
    ch, cw = (H, W) if cells == "grid" else (1, 1)
    if cell_size is not None:
        ch, cw = _cell_size_hw(cell_size)
    grid = (-(-H // ch), -(-W // cw))
    only_cells = cells == "map" and cell_size is not None
    if weight is None:
        if only_cells:
            raise ValueError("cell_size only has a meaning together with a per-cell weight")
        return L.MA_SMOOTH_WEIGHT_NONE, ch, cw
    if not isinstance(weight, (np.ndarray, DeviceArray)):
        raise ValueError(f"weight must be a numpy array or a DeviceArray, got {type(weight).__name__}")
    wshape, wdtype = tuple(weight.shape), weight.dtype
    if not only_cells and wshape == (H, W) and wdtype == np.float32:
        return L.MA_SMOOTH_WEIGHT_F32, ch, cw
    if not only_cells and wshape == (H, W) and wdtype == np.uint8:
        return L.MA_SMOOTH_WEIGHT_U8, ch, cw
    if cell_size is not None and wshape == grid and wdtype == np.float32:
        return L.MA_SMOOTH_WEIGHT_CELLS, ch, cw
    if only_cells:
        raise ValueError(f"a per-cell weight of cells {(ch, cw)} must be float32 of shape {grid}, got {wdtype} {wshape}")
    per_cell = f", or float32 of shape {grid} for cells {(ch, cw)}" if cell_size is not None else ""
    raise ValueError(f"a per-pixel weight must be float32 or uint8 of shape {(H, W)}{per_cell}, got {wdtype} {wshape}")


def _want_and_cells(want, planes, cell_size):
    """(cell_h, cell_w or None twice, want as a tuple) of a call that makes the planes named in `want` and, with cell_size,
    per-cell counts"""
    if isinstance(want, str) or not all(isinstance(n, str) and n in planes for n in want) or \
            len(set(want)) != len(tuple(want)):
        raise ValueError(f"want must name distinct planes among {planes}, got {want!r}")
    if not tuple(want) and cell_size is None:
        raise ValueError("no output was asked for")
    return ((None, None) if cell_size is None else _cell_size_hw(cell_size)) + (tuple(want),)


def smooth_flow_params(flow, taps, weight=None, cell_size=None, where="all", min_support=0.0):
    """Checks and host-side arguments of the weighted smoothing (include/microaligner_flowsmooth.h) without touching a
    device: (H, W, taps as C-contiguous float32, r, weight kind, cell_h, cell_w, mode, min_support as float32).
    weight: None; an (H, W) float32 or uint8 array (numpy or device); or, with cell_size, a (gy, gx) float32 map on that
    cell grid.  ValueError for anything the C entry would refuse."""
    H, W = _check_flow(flow)
    taps, r = _check_taps(taps)
    if not isinstance(where, str) or where not in SMOOTH_MODES:
        raise ValueError(f"unknown mode {where!r}: expected one of {sorted(SMOOTH_MODES)}")
    ms = _finite_f32(min_support, "min_support")
    if not ms >= 0:
        raise ValueError(f"min_support must not be negative, got {min_support!r}")
    kind, ch, cw = _weight_kind(weight, H, W, cell_size, "map")
    return H, W, taps, r, kind, ch, cw, SMOOTH_MODES[where], ms


def fold_mask_params(flow, margin):
    """Checks of the fold mask (include/microaligner_flowsmooth.h) without touching a device: (H, W, margin)."""
    H, W = _check_flow(flow)
    if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or not 0 <= int(margin) <= L.MA_FOLD_MASK_MAX_MARGIN:
        raise ValueError(f"margin must be an integer in [0, {L.MA_FOLD_MASK_MAX_MARGIN}], got {margin!r}")
    return H, W, int(margin)


# ---- median filter of a flow, outlier mask (include/microaligner_flowmedian.h) ---------------------------------------------
MEDIAN_MODES = {"all": L.MA_MEDIAN_ALL, "outliers": L.MA_MEDIAN_OUTLIERS}


def median_flow_params(flow, radius=2, weight=None, cell_size=None, where="all", thresh=None, generic=False):
    """Checks and host-side arguments of the median filter (include/microaligner_flowmedian.h) without touching a device:
    (H, W, r, weight kind, cell_h, cell_w, mode, thresh as float32, flags).  weight: what it is for smooth_flow, read as a
    mask.  thresh: None stands for +Inf ("no outliers") and is refused with where="outliers".  ValueError for anything the
    C entry would refuse."""
    H, W = _check_flow(flow)
    if -(-H // 32) * -(-W // 64) > 0x7fffffff:
        raise ValueError(f"flow too large: more than 2^31 - 1 tiles of 32 x 64 pixels in {(H, W)}")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= L.MA_MEDIAN_MAX_RADIUS:
        raise ValueError(f"radius must be an integer in [1, {L.MA_MEDIAN_MAX_RADIUS}], got {radius!r}")
    if not isinstance(where, str) or where not in MEDIAN_MODES:
        raise ValueError(f"unknown mode {where!r}: expected one of {sorted(MEDIAN_MODES)}")
    if thresh is None:
        if where == "outliers":
            raise ValueError('where="outliers" needs a thresh')
        th = np.float32(np.inf)
    else:
        th = _real(thresh, "thresh")
        with np.errstate(over="ignore"):
            th = np.float32(th)
        if not th >= 0:
            raise ValueError(f"thresh must not be NaN or negative, got {thresh!r}")
    if not isinstance(generic, (bool, np.bool_)):
        raise ValueError(f"generic must be a bool, got {generic!r}")
    kind, ch, cw = _weight_kind(weight, H, W, cell_size, "map")
    return H, W, int(radius), kind, ch, cw, MEDIAN_MODES[where], float(th), L.MA_MEDIAN_GENERIC if generic else 0


# ---- push-pull fill of a flow (include/microaligner_flowfill.h) ------------------------------------------------------------
def fill_flow_params(flow, weight=None, cell_size=None):
    """Checks and host-side arguments of the push-pull fill (include/microaligner_flowfill.h) without touching a device:
    (H, W, weight kind, cell_h, cell_w, levels).  weight: what it is for smooth_flow.  levels: the number of pyramid levels
    above the flow.  ValueError for anything the C entry would refuse."""
    H, W = _check_flow(flow)
    if -(-H // 8) * -(-W // 128) > 0x7fffffff:
        raise ValueError(f"flow too large: more than 2^31 - 1 tiles of 8 x 128 pixels in {(H, W)}")
    kind, ch, cw = _weight_kind(weight, H, W, cell_size, "map")
    return H, W, kind, ch, cw, (max(H, W) - 1).bit_length()


# ---- texture support maps of an image (include/microaligner_texture.h) ----------------------------------------------------
TEXTURE_PLANES = ("lam_min", "lam_max", "weight")


def texture_maps_params(img, taps, floor=None, cell_size=None, want=("lam_min", "lam_max")):
    """Checks and host-side arguments of the texture support maps (include/microaligner_texture.h) without touching a
    device: (H, W, dtype code, taps as C-contiguous float32, r, floor as float32 or None, cell_h, cell_w or None twice,
    want as a tuple).  img: an (H, W) uint8, uint16 or float32 array (numpy or device).  want: which of "lam_min", "lam_max"
    and "weight" to make; the weight needs a floor, and so do the per-cell counts that cell_size asks for.  ValueError for
    anything the C entry would refuse."""
    if not isinstance(img, (np.ndarray, DeviceArray)):
        raise ValueError(f"img must be a numpy array or a DeviceArray, got {type(img).__name__}")
    if len(img.shape) != 2:
        raise ValueError(f"expected a 2D grayscale image, got shape {tuple(img.shape)}")
    dtype = _dt(img.dtype)
    H, W = (int(v) for v in img.shape)
    _image_sides(H, W)
    taps, r = _check_taps(taps)
    ch, cw, want = _want_and_cells(want, TEXTURE_PLANES, cell_size)
    if floor is not None:
        floor = _positive_f32(floor, "floor")
    elif "weight" in want or cell_size is not None:
        raise ValueError("the weight and the per-cell counts need a floor")
    return H, W, dtype, taps, r, floor, ch, cw, want


# ---- affine part of a flow (include/microaligner_flowaffine.h) -------------------------------------------------------------
def flow_affine_moments_params(flow, weight=None, cell_size=None, prior=None, clip=None):
    """Checks and host-side arguments of the affine moments (include/microaligner_flowaffine.h) without touching a device:
    (H, W, weight kind, cell_h, cell_w, prior as 6 float64 or None, clip).  cell_size None: one cell, the whole image.
    weight: None; an (H, W) float32 or uint8 array (numpy or device); or, with cell_size, a (gy, gx) float32 map on that
    cell grid.  prior: a finite 2 x 3 matrix in the centred frame, with clip > 0.  ValueError for anything the C entry would
    refuse."""
    H, W = _check_flow(flow)
    kind, ch, cw = _weight_kind(weight, H, W, cell_size, "grid")
    if prior is None:
        if clip is not None:
            raise ValueError("clip only has a meaning together with a prior")
        return H, W, kind, ch, cw, None, 0.0
    pr = _matrix_2x3(prior, "prior")
    c = _real(clip, "clip")
    if not c > 0:
        raise ValueError(f"clip must be > 0, got {clip!r}")
    return H, W, kind, ch, cw, pr, c


def flow_affine_apply_params(flow, mat):
    """Checks of apply(flow, A) (include/microaligner_flowaffine.h) without touching a device: (H, W, A as 6 float64)."""
    H, W = _check_flow(flow)
    return H, W, _matrix_2x3(mat, "the matrix")


# ---- intensity-based affine alignment (include/microaligner_direct.h) ------------------------------------------------------
def _check_image(img, name):
    if not isinstance(img, (np.ndarray, DeviceArray)):
        raise ValueError(f"{name} must be a numpy array or a DeviceArray, got {type(img).__name__}")
    if len(img.shape) != 2:
        raise ValueError(f"{name}: expected a 2D grayscale image, got shape {tuple(img.shape)}")
    return _dt(img.dtype)


def direct_affine_moments_params(ref, mov, M, gain=1.0, bias=0.0, weight=None, clip=None):
    """Checks and host-side arguments of the alignment moments (include/microaligner_direct.h) without touching a device:
    (H, W, ref dtype code, mov dtype code, M as 6 float64, gain, bias, weight kind, clip as the C entry reads it: 0.0 for
    none).  ref, mov: (H, W) uint8, uint16 or float32 arrays (numpy or device) of one shape.  M: a finite 2 x 3 matrix from
    reference pixels to moving-image pixels.  weight: None, or an (H, W) float32 map or uint8 mask; a per-cell map is
    refused.  clip: None, or a number > 0.  ValueError for anything the C entry would refuse."""
    rdt, mdt = _check_image(ref, "ref"), _check_image(mov, "mov")
    H, W = (int(v) for v in ref.shape)
    if tuple(mov.shape) != (H, W):
        raise ValueError(f"ref and mov must have one shape, got {tuple(ref.shape)} and {tuple(mov.shape)}")
    _image_sides(H, W)
    m = _matrix_2x3(M, "M")
    gain, bias = _real(gain, "gain"), _real(bias, "bias")
    if not (np.isfinite(gain) and np.isfinite(bias)):
        raise ValueError(f"gain and bias must be finite, got {gain!r}, {bias!r}")
    kind = _weight_kind(weight, H, W)[0]
    c = 0.0
    if clip is not None:
        c = _real(clip, "clip")
        if not c > 0:
            raise ValueError(f"clip must be > 0, got {clip!r}")
    return H, W, rdt, mdt, m, gain, bias, kind, c


# ---- refining a flow against the images (include/microaligner_flowrefine.h) ------------------------------------------------
def flow_refine_step_params(ref, warped, flow, taps, floor, weight=None, max_step=1.0):
    """Checks and host-side arguments of one refinement step (include/microaligner_flowrefine.h) without touching a device:
    (H, W, ref dtype code, taps as C-contiguous float32, r, floor as float32, weight kind, max_step as float32).  ref: an
    (H, W) uint8, uint16 or float32 array (numpy or device); warped: (H, W) float32; flow: (H, W, 2) float32; weight: None, or
    an (H, W) float32 map or uint8 mask.  ValueError for anything the C entry would refuse."""
    rdt = _check_image(ref, "ref")
    H, W = _check_flow(flow)
    if tuple(ref.shape) != (H, W):
        raise ValueError(f"ref must have the flow's (H, W) = {(H, W)}, got {tuple(ref.shape)}")
    if not isinstance(warped, (np.ndarray, DeviceArray)) or warped.dtype != np.float32 or tuple(warped.shape) != (H, W):
        raise ValueError(f"warped must be float32 of shape {(H, W)}, got {getattr(warped, 'dtype', None)} "
                         f"{tuple(getattr(warped, 'shape', ()))}")
    taps, r = _check_taps(taps)
    floor, max_step = _positive_f32(floor, "floor"), _positive_f32(max_step, "max_step")
    kind = _weight_kind(weight, H, W)[0]
    return H, W, rdt, taps, r, floor, kind, max_step


# ---- local correlation maps of a registered pair (include/microaligner_localcorr.h) ----------------------------------------
LOCALCORR_PLANES = ("score", "weight")


def local_correlation_params(ref, img, taps, floor, center=(0.0, 0.0), weight=None, lo=0.25, hi=0.75, min_support=0.0,
                             cell_size=None, want=("score",)):
    """Checks and host-side arguments of the local correlation maps (include/microaligner_localcorr.h) without touching a
    device: (H, W, ref dtype code, taps as C-contiguous float32, r, (center_ref, center_img), floor, weight kind,
    min_support, lo, hi -- all as float32 --, cell_h, cell_w or None twice, want as a tuple).  ref: an (H, W) uint8, uint16
    or float32 array (numpy or device); img: (H, W) float32; weight: None, or an (H, W) float32 map or uint8 mask; want: which
    of "score" and "weight" to make.  ValueError for anything the C entry would refuse."""
    rdt = _check_image(ref, "ref")
    H, W = (int(v) for v in ref.shape)
    _image_sides(H, W)
    if not isinstance(img, (np.ndarray, DeviceArray)) or img.dtype != np.float32 or tuple(img.shape) != (H, W):
        raise ValueError(f"img must be float32 of shape {(H, W)}, got {getattr(img, 'dtype', None)} "
                         f"{tuple(getattr(img, 'shape', ()))}")
    taps, r = _check_taps(taps)
    floor = _positive_f32(floor, "floor")
    try:
        ca, cb = center
    except (TypeError, ValueError):
        raise ValueError(f"center must be a pair of numbers, got {center!r}") from None
    ca, cb = _finite_f32(ca, "center[0]"), _finite_f32(cb, "center[1]")
    ms = _finite_f32(min_support, "min_support")
    if not ms >= 0:
        raise ValueError(f"min_support must not be negative, got {min_support!r}")
    lo, hi = _finite_f32(lo, "lo"), _finite_f32(hi, "hi")
    if not -1.0 <= lo < hi <= 1.0:
        raise ValueError(f"lo and hi must satisfy -1 <= lo < hi <= 1 as float32, got {lo!r}, {hi!r}")
    kind = _weight_kind(weight, H, W)[0]
    ch, cw, want = _want_and_cells(want, LOCALCORR_PLANES, cell_size)
    return H, W, rdt, taps, r, (ca, cb), floor, kind, ms, lo, hi, ch, cw, want


# ---- local contrast normalisation of an image (include/microaligner_localnorm.h) -------------------------------------------
LOCALNORM_PLANES = ("u8", "f32")


class LocalNormInfo(collections.namedtuple("LocalNormInfo", "dropped unsupported flat clipped")):
    """normalize_local(..., return_info=True): whole-image counts.  dropped: pixels that are not finite or whose weight is
    not finite and positive; unsupported: live pixels whose window's weight is not above min_support, or whose z is NaN
    (both kinds come out as "no contrast": 0.0 / 128); flat: supported pixels whose local variance is <= floor; clipped:
    supported pixels with |z| > clip."""


def local_norm_params(img, taps, floor, clip=4.0, weight=None, min_support=0.0, want=("u8",)):
    """Checks and host-side arguments of the local contrast normalisation (include/microaligner_localnorm.h) without
    touching a device: (H, W, dtype code, taps as C-contiguous float32, r, floor, clip, weight kind, min_support -- the
    three scalars as float32 --, want as a tuple).  img: an (H, W) uint8, uint16 or float32 array (numpy or device); weight:
    None, or an (H, W) float32 map or uint8 mask; want: which of "u8" and "f32" to make, at least one; clip may be +Inf
    only without "u8".  ValueError for anything the C entry would refuse."""
    dtype = _check_image(img, "img")
    H, W = (int(v) for v in img.shape)
    _image_sides(H, W)
    taps, r = _check_taps(taps)
    floor = _positive_f32(floor, "floor")
    with np.errstate(over="ignore"):
        c = float(np.float32(_real(clip, "clip")))
    if not c > 0:
        raise ValueError(f"clip must be > 0 as float32 and not NaN, got {clip!r}")
    ms = _finite_f32(min_support, "min_support")
    if not ms >= 0:
        raise ValueError(f"min_support must not be negative, got {min_support!r}")
    kind = _weight_kind(weight, H, W)[0]
    if not isinstance(want, (tuple, list)) or not all(isinstance(n, str) and n in LOCALNORM_PLANES for n in want) or \
            len(set(want)) != len(want) or not want:
        raise ValueError(f"want must name one or both of {LOCALNORM_PLANES}, got {want!r}")
    if "u8" in want and np.isinf(c):
        raise ValueError("an infinite clip has no uint8 output: ask for \"f32\" alone")
    return H, W, dtype, taps, r, floor, c, kind, ms, tuple(want)


# ---- flat grey morphology of an image (include/microaligner_morphology.h) ---------------------------------------------------
MORPH_OPS = {"erode": L.MA_MORPH_ERODE, "dilate": L.MA_MORPH_DILATE, "open": L.MA_MORPH_OPEN, "close": L.MA_MORPH_CLOSE,
             "tophat": L.MA_MORPH_TOPHAT, "blackhat": L.MA_MORPH_BLACKHAT}


def morphology_params(img, op, radius):
    """Checks and host-side arguments of the flat grey morphology (include/microaligner_morphology.h) without touching a
    device: (H, W, dtype code, op code, ry, rx).  img: an (H, W) uint8, uint16 or float32 array (numpy or device), not
    empty; op: one of "erode", "dilate", "open", "close", "tophat", "blackhat"; radius: an int, or (ry, rx), each an int
    in 0 .. 255 (the rectangle has (2 ry + 1) x (2 rx + 1) pixels).  ValueError for anything the C entry would refuse."""
    dtype = _check_image(img, "img")
    H, W = (int(v) for v in img.shape)
    _image_sides(H, W)
    if not isinstance(op, str) or op not in MORPH_OPS:
        raise ValueError(f"op must be one of {sorted(MORPH_OPS)}, got {op!r}")
    rr = radius
    if isinstance(rr, (int, np.integer)) and not isinstance(rr, (bool, np.bool_)):
        rr = (rr, rr)
    if not isinstance(rr, (tuple, list)) or len(rr) != 2 or \
            any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in rr):
        raise ValueError(f"radius must be an int or a pair of ints (ry, rx), got {radius!r}")
    ry, rx = (int(v) for v in rr)
    if not (0 <= ry <= L.MA_MORPH_MAX_RADIUS and 0 <= rx <= L.MA_MORPH_MAX_RADIUS):
        raise ValueError(f"a radius must be in [0, {L.MA_MORPH_MAX_RADIUS}], got {radius!r}")
    return H, W, dtype, MORPH_OPS[op], ry, rx


# ---- connected components of an image (include/microaligner_components.h) ----------------------------------------------------
CC_DTYPES = {np.dtype(np.uint8): L.MA_U8, np.dtype(np.uint16): L.MA_U16, np.dtype(np.int32): L.MA_CC_I32}


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def components_params(img, connectivity=1, by_value=False):
    """Checks and host-side arguments of the connected components (include/microaligner_components.h) without touching a
    device: (H, W, dtype code, flags).  img: an (H, W) uint8, uint16 or int32 array (numpy or device; a numpy bool array is
    taken as uint8), 1 <= H, W <= 2^24 and H * W <= 2^31 - 1; connectivity: 1 (the 4 edge neighbours) or 2 (the 8
    neighbours); by_value: a bool.  ValueError for anything the C entries would refuse."""
    if not isinstance(img, (np.ndarray, DeviceArray)):
        raise ValueError(f"img must be a numpy array or a DeviceArray, got {type(img).__name__}")
    if len(img.shape) != 2:
        raise ValueError(f"img: expected a 2D image, got shape {tuple(img.shape)}")
    dtype = np.dtype(img.dtype)
    if dtype == np.bool_ and isinstance(img, np.ndarray):
        dtype = np.dtype(np.uint8)
    if dtype not in CC_DTYPES:
        raise ValueError(f"unsupported image dtype {dtype}: connected components take uint8, uint16, int32 or a bool mask "
                         "(threshold a float image first)")
    H, W = (int(v) for v in img.shape)
    _image_sides(H, W)
    if H * W > L.MA_CC_MAX_PIXELS:
        raise ValueError(f"image too large: H * W must be at most 2^31 - 1, got {H} x {W}")
    if not _is_int(connectivity) or connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 or 2, got {connectivity!r}")
    if not isinstance(by_value, (bool, np.bool_)):
        raise ValueError(f"by_value must be a bool, got {by_value!r}")
    flags = (L.MA_CC_CONN8 if connectivity == 2 else 0) | (L.MA_CC_BY_VALUE if by_value else 0)
    return H, W, CC_DTYPES[dtype], flags


def remove_small_params(img, min_size, connectivity=1, by_value=False):
    """components_params and min_size, an int >= 0: (H, W, dtype code, flags, min_size)."""
    H, W, dtype, flags = components_params(img, connectivity, by_value)
    if not _is_int(min_size) or min_size < 0:
        raise ValueError(f"min_size must be an int >= 0, got {min_size!r}")
    return H, W, dtype, flags, int(min_size)


def fill_holes_params(img, max_size=None, connectivity=1, value=1):
    """components_params, max_size (None or an int >= 0) and value (an int in 1 .. the largest value of img's dtype):
    (H, W, dtype code, flags, max_area as the C entry reads it, value)."""
    H, W, dtype, flags = components_params(img, connectivity, False)
    if max_size is not None and (not _is_int(max_size) or max_size < 0):
        raise ValueError(f"max_size must be None or an int >= 0, got {max_size!r}")
    top = {L.MA_U8: 255, L.MA_U16: 65535, L.MA_CC_I32: 2 ** 31 - 1}[dtype]
    if not _is_int(value) or not 1 <= value <= top:
        raise ValueError(f"value must be an int in [1, {top}], got {value!r}")
    max_area = L.MA_CC_MAX_PIXELS if max_size is None else min(int(max_size), L.MA_CC_MAX_PIXELS)
    return H, W, dtype, flags | L.MA_CC_HOLES, max_area, int(value)


# ---- global translation search (include/microaligner_translation.h) --------------------------------------------------------
def translation_params(ref, mov, window, exclude=0):
    """Checks and host-side arguments of the translation search (include/microaligner_translation.h) without touching a
    device: (h, w, dx0, dx1, dy0, dy1, exclude).  ref, mov: (h, w) uint8 labels (numpy or device) of one shape; window:
    (dx0, dx1, dy0, dy1), both ends included, at most 2^20 shifts; exclude: an int >= 0.  ValueError for anything the C
    entries would refuse."""
    for img, name in ((ref, "ref"), (mov, "mov")):
        _check_image(img, name)
        if img.dtype != np.uint8:
            raise ValueError(f"{name} must be uint8 labels, got {img.dtype}")
    h, w = (int(v) for v in ref.shape)
    if tuple(mov.shape) != (h, w):
        raise ValueError(f"ref and mov must have one shape, got {tuple(ref.shape)} and {tuple(mov.shape)}")
    if h < 1 or w < 1 or h * w > L.MA_TRANSLATION_MAX_PIXELS:
        raise ValueError(f"an image must hold 1 .. 2^32 pixels, got {(h, w)}")
    try:
        win = [v for v in window]
    except TypeError:
        raise ValueError("window must be (dx0, dx1, dy0, dy1)") from None
    if len(win) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in win):
        raise ValueError(f"window must be four ints (dx0, dx1, dy0, dy1), got {window!r}")
    dx0, dx1, dy0, dy1 = (int(v) for v in win)
    if any(abs(v) >= 1 << 31 for v in (dx0, dx1, dy0, dy1)):
        raise ValueError(f"window out of the int range: {window!r}")
    if dx1 < dx0 or dy1 < dy0:
        raise ValueError(f"empty window {window!r}")
    if (dx1 - dx0 + 1) * (dy1 - dy0 + 1) > L.MA_TRANSLATION_MAX_SHIFTS:
        raise ValueError(f"a window must hold at most 2^20 shifts, got {(dx1 - dx0 + 1) * (dy1 - dy0 + 1)}")
    if isinstance(exclude, bool) or not isinstance(exclude, (int, np.integer)) or not 0 <= exclude < 1 << 31:
        raise ValueError(f"exclude must be an int >= 0, got {exclude!r}")
    return h, w, dx0, dx1, dy0, dy1, int(exclude)


# ---- order statistics and range normalisation (include/microaligner_quantile.h) -------------------------------------------
def image_quantiles_params(arr, q, ignore_zeros=False):
    """Checks and host-side arguments of Context.image_quantiles (include/microaligner_quantile.h) without touching a
    device: (dtype code, n, q as a float64 array, flags).  arr: a uint8 / uint16 / float32 array (numpy or device) of 1 ..
    2^40 elements; q: one number or 1 .. 8 of them, each in [0, 1], in any order; ignore_zeros: a bool.  ValueError for
    anything the C entry would refuse."""
    if not hasattr(arr, "dtype") or not hasattr(arr, "shape") or np.dtype(arr.dtype) not in _DT:
        raise ValueError(f"expected a uint8 / uint16 / float32 array, got {getattr(arr, 'dtype', type(arr))}")
    n = 1
    for v in arr.shape:
        n *= int(v)
    if not 1 <= n <= L.MA_Q_MAX_PIXELS:
        raise ValueError(f"an image must hold 1 .. 2^40 pixels, got shape {tuple(arr.shape)}")
    try:
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"q must be numbers in [0, 1], got {q!r}") from None
    if qs.ndim != 1 or not 1 <= qs.size <= L.MA_Q_MAX_RANKS:
        raise ValueError(f"q must hold 1 .. {L.MA_Q_MAX_RANKS} numbers, got {q!r}")
    if not np.all((qs >= 0.0) & (qs <= 1.0)):              # false for a NaN
        raise ValueError(f"every q must lie in [0, 1], got {q!r}")
    if not isinstance(ignore_zeros, (bool, np.bool_)):
        raise ValueError(f"ignore_zeros must be a bool, got {ignore_zeros!r}")
    return _DT[np.dtype(arr.dtype)], n, np.ascontiguousarray(qs), L.MA_Q_IGNORE_ZEROS if ignore_zeros else 0


def normalize_range_params(arr, lo, hi):
    """Checks of Context.normalize_range_u8 without touching a device: (dtype code, n, lo, hi) with lo and hi finite
    floats.  ValueError otherwise."""
    if not hasattr(arr, "dtype") or not hasattr(arr, "shape") or np.dtype(arr.dtype) not in _DT:
        raise ValueError(f"expected a uint8 / uint16 / float32 array, got {getattr(arr, 'dtype', type(arr))}")
    n = 1
    for v in arr.shape:
        n *= int(v)
    if n < 1:
        raise ValueError(f"empty array of shape {tuple(arr.shape)}")
    lo, hi = _real(lo, "lo"), _real(hi, "hi")
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"lo and hi must be finite, got {lo!r} and {hi!r}")
    return _DT[np.dtype(arr.dtype)], n, lo, hi


# ---- what the calls above report -------------------------------------------------------------------------------------------
class SmoothInfo(collections.namedtuple("SmoothInfo", "unsupported")):
    """smooth_flow(..., return_info=True): the number of pixels whose smoothed value had no support (S2 <= min_support)."""


class FoldInfo(collections.namedtuple("FoldInfo", "folded invalid dropped")):
    """fold_mask(..., return_info=True): pixels with a finite det J <= 0, pixels with a non-finite component (the sums of
    flow_qc's maps), and pixels the mask drops (keep == 0)."""


class MedianInfo(collections.namedtuple("MedianInfo", "outliers dropped unsupported")):
    """median_flow(..., return_info=True): participating pixels farther than thresh from the median of their window,
    pixels that do not participate (weight or value), and those of them whose window holds no participating pixel at all
    (their median is NaN)."""


class FillInfo(collections.namedtuple("FillInfo", "dropped blended unsupported levels")):
    """fill_flow(..., return_info=True): pixels that were filled (weight NaN, negative or 0, or a flow that is not finite),
    pixels blended with the fill (a weight in (0, 1)), output pixels with a non-finite component (all of them where every
    pixel was dropped), and the number of pyramid levels above the flow."""


class RepairInfo(collections.namedtuple("RepairInfo", "rounds converged")):
    """repair_flow(..., return_info=True): (folded, invalid, dropped, unsupported) of every smoothing round, and whether
    the loop ended on a flow with nothing folded and nothing invalid."""


class RefineStepInfo(collections.namedtuple("RefineStepInfo", "step_max clamped invalid")):
    """Context.flow_refine_step(..., return_info=True): the largest |component| of the step in px (after the clamp), the
    pixels where the clamp changed a component, and the pixels whose system had no solution (their step is 0)."""


class FlowRefineInfo(collections.namedtuple("FlowRefineInfo", "steps iterations converged")):
    """refine_flow(..., return_info=True): the RefineStepInfo (step_max, clamped, invalid) of every step taken, their
    number, and whether the loop ended on a step with step_max <= tol."""


class QuantileCounts(collections.namedtuple("QuantileCounts", "pop nonfinite zeros")):
    """Context.image_quantiles: the pixels of the population, the NaN / +-Inf pixels left out of it, and the zeros left out
    with ignore_zeros.  pop + nonfinite + zeros is the size of the image."""


class InvertInfo(collections.namedtuple("InvertInfo", "not_converged residual")):
    """invert_flow(..., return_info=True): the number of pixels that took max_iter steps without stopping, and the (H, W)
    float32 size of every pixel's last step (NaN where it was NaN)."""


class PointsInfo(collections.namedtuple("PointsInfo", "converged inside")):
    """transform_points(..., return_info=True): per point, whether the iteration stopped (always True for "to_moving"
    and a finite point), and whether the registered-frame coordinate lies inside the flow's grid."""


class DeviceArray:
    """Dense row-major array living in HBM.  Freed back to the context's pool on `free()`/GC."""

    __slots__ = ("ctx", "shape", "dtype", "ptr", "_nbytes_alloc", "_owner", "minmax", "cellkeys")

    def __init__(self, ctx, shape, dtype, ptr, nbytes_alloc, owner=True):
        self.ctx, self.shape, self.dtype, self.ptr = ctx, tuple(int(s) for s in shape), np.dtype(dtype), ptr
        self._nbytes_alloc, self._owner = nbytes_alloc, owner
        # optional DeviceArray of two floats (min, max of this array), left by the kernel that produced it
        # (Context.warp / pyr_down with minmax=True) for a following dog_u8; arrays are never modified in place
        self.minmax = None
        # optional (tile, overlap, DeviceArray of keys): per-cell maxima of this FLOW, left by a warp that read it
        # (Context.warp(flow_cells=True)) for a following merge_flows
        self.cellkeys = None

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def ndim(self):
        return len(self.shape)

    def __len__(self):
        return self.shape[0] if self.shape else 0

    def numpy(self, out=None):
        """Copy to the host.  Without `out` the result array comes from the context's pool of page-locked,
        already-faulted host buffers (Context.host_empty): an ordinary ndarray whose memory goes back to the pool
        when the last reference to it (or to a view of it) is dropped.  `out`: a C-contiguous array of the same
        shape and dtype to fill instead (e.g. a row of the caller's memmap)."""
        self._check_alive()
        own = out is None
        if own:
            out = self.ctx.host_empty(self.shape, self.dtype)
        elif (tuple(out.shape) != self.shape or out.dtype != self.dtype or not out.flags.c_contiguous
              or not out.flags.writeable):
            raise ValueError(f"out must be a writable C-contiguous {self.dtype} array of shape {self.shape}")
        if out.nbytes:
            L.check(self.ctx.lib.ma_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes))
        if own and self.ctx._resident.mode == "results":
            # results are handed out read-only (the flags of a caller's `out` array are never touched): that is what
            # lets asdevice(out) find this device array again instead of uploading the bytes it has just downloaded
            self.ctx._resident.freeze(out)
        self.ctx._resident.remember(out, self)
        return out

    def _check_alive(self):
        if self.ptr is None or self.ctx is None or self.ctx._closed:
            raise RuntimeError("this DeviceArray was freed (its context is closed or free() was called)")

    def copy(self):
        out = self.ctx.empty(self.shape, self.dtype)
        L.check(self.ctx.lib.ma_memcpy_d2d(self.ctx.handle, out.ptr, self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr and self._owner and self.ctx is not None:
            self.ctx._release(self.ptr, self._nbytes_alloc)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- grid flows (include/microaligner_flowgrid.h) ------------------------------------------------------------------------
def grid_nodes(n, stride):
    """g(n, s): the number of nodes of an axis of n pixels at stride s -- 1 for one pixel, else ceil((n - 1) / s) + 1."""
    return 1 if n == 1 else -(-(n - 1) // stride) + 1


def _check_stride(stride):
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= int(stride) < 1 << 31:
        raise ValueError(f"stride must be an integer in [1, 2^31), got {stride!r}")
    return int(stride)


def _check_grid_shape(shape):
    try:
        H, W = shape
        ok = all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 1 <= int(v) <= 1 << 30 for v in (H, W))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"shape must be the flow's (H, W) with sides in [1, 2^30], got {shape!r}")
    return int(H), int(W)


class FlowGrid:
    """A flow kept as its values on a coarse grid: `nodes` (gh, gw, 2) float32, one node every `stride` pixels of a flow of
    `shape` (H, W) and one on the last row and column, bilinear interpolation between them
    (include/microaligner_flowgrid.h).  nodes: a numpy array or a DeviceArray.  ValueError for a wrong dtype, stride or
    shape, or nodes that are not (g(H, s), g(W, s), 2), before any device work."""
    FORMAT_VERSION = 1

    def __init__(self, nodes, stride, shape):
        self.stride, self.shape = _check_stride(stride), _check_grid_shape(shape)
        want = (grid_nodes(self.shape[0], self.stride), grid_nodes(self.shape[1], self.stride), 2)
        if not isinstance(nodes, (np.ndarray, DeviceArray)) or nodes.dtype != np.float32 or tuple(nodes.shape) != want:
            raise ValueError(f"nodes must be a float32 numpy array or DeviceArray of shape {want} for a flow of shape "
                             f"{self.shape} at stride {self.stride}, got {getattr(nodes, 'dtype', type(nodes))} "
                             f"{tuple(getattr(nodes, 'shape', ()))}")
        self.nodes = nodes if isinstance(nodes, DeviceArray) else np.ascontiguousarray(nodes)

    def __len__(self):
        return self.nodes.shape[0]

    def __repr__(self):
        return f"FlowGrid(shape={self.shape}, stride={self.stride}, nodes={tuple(self.nodes.shape)})"

    @property
    def nbytes(self):
        return int(self.nodes.nbytes)

    def expand(self):
        """The dense (H, W, 2) float32 flow, evaluated on the device: numpy nodes give numpy, device nodes a DeviceArray."""
        out = get_context().flow_grid_expand(self)
        return out if isinstance(self.nodes, DeviceArray) else out.numpy()

    def save(self, path):
        """Write nodes, stride, shape and the format version to a .npz (numpy appends the suffix if `path` lacks it)."""
        nodes = self.nodes.numpy() if isinstance(self.nodes, DeviceArray) else self.nodes
        np.savez(path, nodes=nodes, stride=np.int64(self.stride), shape=np.asarray(self.shape, np.int64),
                 format_version=np.int64(self.FORMAT_VERSION))

    @classmethod
    def load(cls, path):
        """The grid save() wrote (numpy nodes).  ValueError for a file that is not one or has another format version."""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("nodes", "stride", "shape", "format_version") if k not in z.files]
            if missing:
                raise ValueError(f"{path} is not a FlowGrid file: {missing} missing")
            version = int(z["format_version"])
            if version != cls.FORMAT_VERSION:
                raise ValueError(f"{path} has FlowGrid format version {version}, this package reads {cls.FORMAT_VERSION}")
            return cls(z["nodes"], int(z["stride"]), tuple(int(v) for v in z["shape"]))


def dense_flow(flow):
    """The one place a FlowGrid becomes a dense flow for the calls that have no native grid path (invert_flow,
    compose_flows, flow_qc): expanded on the device, a DeviceArray.  Anything else passes through."""
    return get_context().flow_grid_expand(flow) if isinstance(flow, FlowGrid) else flow


def affine_grid_params(img_shape, img_dtype, grid, tmat, interpolation="linear"):
    """affine_flow_params for a FlowGrid.  tmat None: the identity and no padding, so the image has the grid's (H, W)."""
    if not isinstance(grid, FlowGrid):
        raise ValueError(f"expected a FlowGrid, got {type(grid).__name__}")
    H, W = grid.shape
    if tmat is not None:
        return affine_flow_params(img_shape, img_dtype, (H, W, 2), np.float32, tmat, interpolation)
    interp = interp_code(interpolation)
    _dt(img_dtype)
    if tuple(img_shape) != (H, W):
        raise ValueError(f"without tmat the image must have the grid's shape {(H, W)}, got {tuple(img_shape)}")
    return interp, np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), 0, 0


# ---- thin-plate spline of landmark pairs (include/microaligner_landmarks.h) -----------------------------------------------
def _check_spline(cw, a6, c, k):
    if not isinstance(cw, np.ndarray) or cw.dtype != np.float64 or cw.ndim != 2 or cw.shape[1] != 4:
        raise ValueError("cw must be an (n, 4) float64 numpy array of (u.x, u.y, w.x, w.y)")
    if cw.shape[0] > L.MA_LANDMARK_MAX:
        raise ValueError(f"at most {L.MA_LANDMARK_MAX} landmarks per call, got {cw.shape[0]}")
    try:
        a6 = np.asarray(a6, dtype=np.float64).ravel()
        c = np.asarray(c, dtype=np.float64).ravel()
        k = float(k)
    except (TypeError, ValueError) as e:
        raise ValueError(f"the affine part, the centre and the scale must be numbers: {e}") from None
    if a6.shape != (6,) or c.shape != (2,):
        raise ValueError(f"the affine part must hold 6 values and the centre 2, got {a6.size} and {c.size}")
    if not (np.all(np.isfinite(cw)) and np.all(np.isfinite(a6)) and np.all(np.isfinite(c)) and np.isfinite(k)):
        raise ValueError("the landmark records, the affine part, the centre and the scale must be finite")
    return np.ascontiguousarray(cw), a6, float(c[0]), float(c[1]), k


def landmark_flow_params(cw, a6, c, k, shape, stride=1):
    """Checks and host-side arguments of the spline on a grid (include/microaligner_landmarks.h) without touching a device:
    (cw as a C-contiguous (n, 4) float64 array, a6 as 6 float64, cx, cy, k, H, W, stride).  ValueError for anything the C
    entry would refuse, and for non-finite records."""
    spline = _check_spline(cw, a6, c, k)
    H, W = _check_grid_shape(shape)
    if H > 1 << 24 or W > 1 << 24:
        raise ValueError(f"flow sides must be in [1, 2^24], got {(H, W)}")
    return spline + (H, W, _check_stride(stride))


def landmark_points_params(cw, a6, c, k, points):
    """Checks and host-side arguments of the spline at points without touching a device: the spline as
    landmark_flow_params gives it, and the points as a C-contiguous (N, 2) float64 array."""
    spline = _check_spline(cw, a6, c, k)
    if not isinstance(points, np.ndarray) or points.dtype != np.float64 or points.ndim != 2 or points.shape[1] != 2:
        raise ValueError("points must be an (N, 2) float64 numpy array of (x, y)")
    if points.shape[0] >= 1 << 31:
        raise ValueError("at most 2^31 - 1 points per call")
    return spline + (np.ascontiguousarray(points),)


class _HostBuffer:
    """Owner of one page-locked host buffer; exposes it through __array_interface__ so that numpy arrays built on
    it keep it alive (base chain), and hands the memory back to the pool when it dies."""

    __slots__ = ("ctx", "ptr", "bucket", "nbytes", "__weakref__")   # weakly referenced by the resident-pair cache

    def __init__(self, ctx, ptr, bucket, nbytes):
        self.ctx, self.ptr, self.bucket, self.nbytes = ctx, ptr, bucket, nbytes

    @property
    def __array_interface__(self):        # numpy (any Python): zero-copy view, base object = self
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            self.ctx._host_release(self.ptr, self.bucket)
        except Exception:
            pass


class _ResidentCache:
    """Host array <-> device array pairs that are known to hold the same bytes.

    The reference's callers move every array through numpy: register() returns the flow, the very next statement
    hands it to Warper (microaligner/__main__.py:418-433), and warp_and_save_pages sets the same flow on the warper
    for every page of a cycle (:296-301).  Through a drop-in API that is one 2.1 GB upload per call at 16384^2.  This
    cache lets Context.asdevice() recognise a host array whose bytes are already on the device and return the device
    array that is still alive instead.  An entry is only ever made for memory that CANNOT have changed since:

      * key: address, shape, strides and dtype of the host array (C-contiguous arrays of at least MIN_BYTES only);
      * liveness: a weak reference to the object that owns the memory (the end of the array's .base chain); when it
        dies the entry goes with it, so a recycled address can never match;
      * immutability (mode "results", the default): the arrays DeviceArray.numpy() hands out -- the flow of register(),
        the image of warp() -- are marked read-only down to the root of their base chain, so an in-place edit raises
        (numpy: "assignment destination is read-only") instead of going unnoticed; take a .copy() to edit one.  Arrays
        of the caller are recorded only when they are read-only themselves (np.memmap(mode="r"), arr.flags.writeable =
        False on the owner).  A hit requires every array of the base chain to be read-only still;
      * bound: least recently used pairs are dropped beyond MICROALIGNER_RESIDENT_GB (default 16) of device memory.

    MICROALIGNER_RESIDENT=off: no cache, results are ordinary writable arrays (everything is uploaded every time).
    MICROALIGNER_RESIDENT=sampled: results stay writable and ANY uploaded array is recorded, guarded by a CRC of head,
    tail and SAMPLES strided bytes checked on every hit -- cheap, but NOT sound: an in-place edit of a block that falls
    between the samples (stride ~256 KiB at 2 GB) goes unnoticed and the stale device copy is used.  Opt-in only, for
    callers that never edit arrays in place.

    Device arrays are never modified in place (every operation allocates its output), so a recorded pair stays valid
    for as long as the host side is untouched."""

    MIN_BYTES = 1 << 20
    SAMPLES = 8192
    EDGE = 4096

    def __init__(self):
        self.mode = os.environ.get("MICROALIGNER_RESIDENT", "results").lower()
        if self.mode == "readonly":      # earlier name of the default mode
            self.mode = "results"
        if self.mode not in ("results", "sampled", "off"):
            raise ValueError("MICROALIGNER_RESIDENT must be one of results, sampled, off")
        self.limit = int(float(os.environ.get("MICROALIGNER_RESIDENT_GB", "16")) * (1 << 30))
        self.entries = collections.OrderedDict()   # key -> [weakref(owner), DeviceArray, signature]
        self.bytes = 0
        self.hits = 0
        # weak-reference callbacks (_forget) run from the collector on whichever thread it picks, and the engines of
        # parallel.stream_pairs run on their own threads; re-entrant: a callback can fire inside remember() / lookup()
        self.lock = threading.RLock()

    @staticmethod
    def _key(arr):
        return (arr.__array_interface__["data"][0], arr.shape, arr.strides, arr.dtype.str)

    @staticmethod
    def _owner(arr):
        while isinstance(getattr(arr, "base", None), np.ndarray):
            arr = arr.base
        return arr.base if getattr(arr, "base", None) is not None else arr

    @staticmethod
    def _frozen(arr):
        """True when neither `arr` nor any array it is a view of can be written through numpy."""
        while isinstance(arr, np.ndarray):
            if arr.flags.writeable:
                return False
            arr = arr.base
        return True

    @staticmethod
    def freeze(arr):
        """Mark `arr` and every array of its base chain read-only (root first is not needed: clearing the flag is
        always allowed; setting it again is refused by numpy while the root is read-only)."""
        while isinstance(arr, np.ndarray):
            arr.flags.writeable = False
            arr = arr.base

    @classmethod
    def _signature(cls, arr):
        b = arr.reshape(-1).view(np.uint8)
        n = b.size
        step = max(1, n // cls.SAMPLES) | 1
        crc = zlib.crc32(b[:cls.EDGE].tobytes())
        crc = zlib.crc32(b[-cls.EDGE:].tobytes(), crc)
        return zlib.crc32(b[::step].tobytes(), crc)

    def _eligible(self, arr):
        if not (self.mode != "off" and isinstance(arr, np.ndarray) and arr.flags.c_contiguous
                and arr.nbytes >= self.MIN_BYTES):
            return False
        return self.mode == "sampled" or self._frozen(arr)

    def remember(self, arr, dev):
        if not self._eligible(arr) or dev.ptr is None:
            return
        key = self._key(arr)
        try:
            ref = weakref.ref(self._owner(arr), lambda _r, k=key: self._forget(k))
        except TypeError:       # the memory owner cannot be weakly referenced (mmap, bytes): liveness unknown
            return
        sig = self._signature(arr) if self.mode == "sampled" else None
        with self.lock:
            self._forget(key)
            self.entries[key] = [ref, dev, sig]
            self.bytes += dev.nbytes
            while self.bytes > self.limit and len(self.entries) > 1:
                self._forget(next(iter(self.entries)))

    def _forget(self, key):
        with self.lock:
            e = self.entries.pop(key, None)
            if e is not None:
                self.bytes -= e[1].nbytes if e[1].ptr is not None else 0

    def lookup(self, arr):
        if not self._eligible(arr):     # results mode: an array that has become writable again is never a hit
            if self.mode != "off" and isinstance(arr, np.ndarray):
                self._forget(self._key(arr))
            return None
        key = self._key(arr)
        with self.lock:
            e = self.entries.get(key)
            if e is None:
                return None
            ref, dev, sig = e
            if (ref() is None or dev.ptr is None or dev.shape != arr.shape or dev.dtype != arr.dtype
                    or (sig is not None and self._signature(arr) != sig)):
                self._forget(key)
                return None
            self.entries.move_to_end(key)
            self.hits += 1
            return dev

    def clear(self):
        with self.lock:
            self.entries.clear()
            self.bytes = 0


class Context:
    """One per HIP device.  Owns the C-side ma_ctx and a size-bucketed pool of HBM buffers."""

    def __init__(self, device=0):
        self.lib = L.load()
        h = C.c_void_p()
        L.check(self.lib.ma_ctx_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)
        self._pool = {}
        self._live = {}        # ptr -> bucket of every buffer handed out and not yet released
        self._host_pool = {}   # bucket -> [pinned host pointers] (result arrays of the numpy-in / numpy-out API)
        self._host_owned = {}  # bucket -> page-locked buffers this context owns (handed out + pooled)
        self._host_lock = threading.RLock()   # re-entrant: a pinned result array finalised by a GC pass that starts inside
        #                                        _host_release() comes back here on the same thread
        self._resident = _ResidentCache()
        self._closed = False
        lim = os.environ.get("MICROALIGNER_WORKSPACE_GB")
        if lim:
            L.check(self.lib.ma_ctx_set_workspace_limit(self.handle, int(float(lim) * (1 << 30))))

    # -- memory --------------------------------------------------------------------------
    def empty(self, shape, dtype):
        shape = tuple(int(s) for s in shape)
        dtype = np.dtype(dtype)
        nbytes = max(int(np.prod(shape, dtype=np.int64)) * dtype.itemsize, 1)
        bucket = (nbytes + 0xFFFF) & ~0xFFFF
        with self._host_lock:    # _release() runs from __del__, i.e. from whichever thread the collector picks
            free = self._pool.get(bucket)
            ptr = free.pop() if free else None
        if ptr is None:
            p = C.c_void_p()
            rc = self.lib.ma_malloc(self.handle, bucket, C.byref(p))
            if rc == L.MA_ENOMEM:
                self.trim()
                rc = self.lib.ma_malloc(self.handle, bucket, C.byref(p))
            L.check(rc)
            ptr = p.value
        with self._host_lock:
            self._live[ptr] = bucket
        return DeviceArray(self, shape, dtype, ptr, bucket)

    def zeros(self, shape, dtype):
        a = self.empty(shape, dtype)
        L.check(self.lib.ma_memset(self.handle, a.ptr, 0, a.nbytes))
        return a

    def asdevice(self, arr):
        """numpy -> DeviceArray (H2D copy); DeviceArray passes through.  A host array this context has uploaded or
        downloaded before, whose memory is still alive and unmodified (_ResidentCache), maps to the device array that
        already holds it: no copy."""
        if isinstance(arr, DeviceArray):
            return arr
        arr = np.ascontiguousarray(arr)
        _dt(arr.dtype)
        d = self._resident.lookup(arr)
        if d is not None:
            return d
        d = self.empty(arr.shape, arr.dtype)
        if arr.nbytes:
            L.check(self.lib.ma_memcpy_h2d(self.handle, d.ptr, arr.ctypes.data, arr.nbytes))
        self._resident.remember(arr, d)
        return d

    def is_resident(self, arr):
        """Whether asdevice(arr) would find the host array in HBM already (no upload)."""
        return isinstance(arr, DeviceArray) or self._resident.lookup(np.ascontiguousarray(arr)) is not None

    def _release(self, ptr, bucket):
        with self._host_lock:
            if self._closed:
                return   # close() already returned every outstanding buffer to the driver
            self._live.pop(ptr, None)
            self._pool.setdefault(bucket, []).append(ptr)

    def trim(self):
        """Return every pooled buffer (device and host) to the driver."""
        self._resident.clear()
        self.lib.ma_ctx_trim(self.handle)   # the intermediates ma_optflow_register caches on the C side
        with self._host_lock:
            dev_pool, self._pool = self._pool, {}
        for free in dev_pool.values():
            for p in free:
                self.lib.ma_free(self.handle, p)
        with self._host_lock:
            pools, self._host_pool = self._host_pool, {}
            for bucket, free in pools.items():
                self._host_owned[bucket] = self._host_owned.get(bucket, 0) - len(free)
        for free in pools.values():
            for p in free:
                self.lib.ma_host_free(p)

    def _run(self, fn, *args):
        """Call a compute entry point; on MA_ENOMEM hand the cached buffers back to the driver and retry once
        (the pool never shrinks by itself and can hold tens of GB of flow-sized buffers)."""
        rc = fn(self.handle, *args)
        if rc == L.MA_ENOMEM:
            self.trim()
            rc = fn(self.handle, *args)
        L.check(rc)

    # page-locked result arrays ---------------------------------------------------------------
    # Page-locked buffers of one size that a context will own at any time (handed out or pooled).  Pinning is far
    # dearer than a page fault per 4 KiB (hipHostMalloc: ~200 ms per GiB; faulting a fresh pageable array: ~25 ms per GiB), so
    # it only pays for buffers that are reused: a caller that keeps accumulating results gets pageable arrays beyond
    # this number, a loop that drops each result before the next but one reuses the same two buffers forever.
    HOST_PINNED_PER_BUCKET = 2

    def host_empty(self, shape, dtype, limit=None):
        """ndarray on page-locked host memory drawn from a pool (`limit`: page-locked buffers of this size the context
        may own, default HOST_PINNED_PER_BUCKET; parallel.stream_pairs keeps more results in flight).  The memory returns to the pool when the array
        and all views of it are gone (the array's base object is the owner), so a loop that keeps calling
        register() / warp() reuses the same already-faulted, DMA-able buffers instead of paying a page fault per
        4 KiB of every fresh result."""
        shape = tuple(int(s) for s in shape)
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < (1 << 20):          # small results: not worth a pinned allocation
            return np.empty(shape, dtype)
        bucket = (nbytes + 0x1FFFFF) & ~0x1FFFFF
        with self._host_lock:
            free = self._host_pool.get(bucket)
            ptr = free.pop() if free else None
            if ptr is None:
                if self._host_owned.get(bucket, 0) >= (limit or self.HOST_PINNED_PER_BUCKET):
                    return np.empty(shape, dtype)
                self._host_owned[bucket] = self._host_owned.get(bucket, 0) + 1
        if ptr is None:
            p = C.c_void_p()
            rc = self.lib.ma_host_alloc(bucket, C.byref(p))
            if rc != L.MA_OK:           # page-locked memory exhausted: fall back to a pageable array
                with self._host_lock:
                    self._host_owned[bucket] -= 1
                return np.empty(shape, dtype)
            ptr = p.value
        owner = _HostBuffer(self, ptr, bucket, nbytes)
        return np.asarray(owner).view(dtype).reshape(shape)   # base chain ends at `owner`

    def host_reserve(self, shape, dtype, count):
        """Make sure the pool can hand out `count` page-locked arrays of this shape at once (allocating what is missing
        now, in one go: hipHostMalloc takes ~0.2 s per GiB and stalls other HIP calls of the process while it runs, so a
        pipeline does this before its first pair rather than in the middle of the stream)."""
        held = [self.host_empty(shape, dtype, limit=count) for _ in range(count)]
        del held

    def _host_release(self, ptr, bucket):
        with self._host_lock:
            if not self._closed:
                self._host_pool.setdefault(bucket, []).append(ptr)
                return
        self.lib.ma_host_free(ptr)

    def sync(self):
        L.check(self.lib.ma_sync(self.handle))

    def debug_fill_idle(self, byte):
        """Test hook (include/microaligner_debug.h): wait for every stream of this context and of its companion, then set
        every byte of their idle scratch memory -- workspace, free buffers of the C-side cache, the small device buffer and
        the page-locked result buffer -- to `byte` (0 .. 255).  Returns the bytes filled of each of the four kinds."""
        if isinstance(byte, bool) or not isinstance(byte, (int, np.integer)) or not 0 <= int(byte) <= 255:
            raise ValueError(f"byte must be an integer in 0..255, got {byte!r}")
        filled = (C.c_ulonglong * 4)()
        L.check(self.lib.ma_debug_fill_idle(self.handle, int(byte), filled))
        return tuple(int(v) for v in filled)

    # -- options / transfer engines ------------------------------------------------------------
    def set_option(self, option, value):
        L.check(self.lib.ma_ctx_set_option(self.handle, int(option), int(value)))

    def get_option(self, option):
        v = C.c_longlong()
        L.check(self.lib.ma_ctx_get_option(self.handle, int(option), C.byref(v)))
        return v.value

    @property
    def companion_stream(self):
        """Whether ma_optflow_register runs the flow-independent dog() calls on the low-priority companion stream
        (MA_OPT_COMPANION_STREAM, default True).  False: one stream, every kernel alone on the chip (profiling)."""
        return bool(self.get_option(L.MA_OPT_COMPANION_STREAM))

    @companion_stream.setter
    def companion_stream(self, on):
        self.set_option(L.MA_OPT_COMPANION_STREAM, 1 if on else 0)

    def engine_upload(self, dst, arr, engine=L.MA_ENGINE_H2D):
        """Copy the C-contiguous host array `arr` into the DeviceArray `dst` on a transfer engine's stream; returns when
        this copy is complete (the compute stream is not involved: order it with engine_record / engine_wait)."""
        if arr.nbytes != dst.nbytes or not arr.flags.c_contiguous:
            raise ValueError("engine_upload needs a C-contiguous host array of the device array's size")
        _warn_if_staged_on_a_full_node(arr)
        L.check(self.lib.ma_engine_memcpy_h2d(self.handle, int(engine), dst.ptr, arr.ctypes.data, arr.nbytes))

    def engine_download(self, src, out, engine=L.MA_ENGINE_D2H):
        if out.nbytes != src.nbytes or not out.flags.c_contiguous:
            raise ValueError("engine_download needs a C-contiguous host array of the device array's size")
        _warn_if_staged_on_a_full_node(out)
        L.check(self.lib.ma_engine_memcpy_d2h(self.handle, int(engine), out.ctypes.data, src.ptr, out.nbytes))

    def engine_record(self, engine, ev):
        L.check(self.lib.ma_engine_record(self.handle, int(engine), ev))

    def engine_wait(self, engine, ev):
        L.check(self.lib.ma_engine_wait(self.handle, int(engine), ev))

    def engine_sync(self, engine):
        L.check(self.lib.ma_engine_sync(self.handle, int(engine)))

    def event_sync(self, ev):
        L.check(self.lib.ma_event_sync(self.handle, ev))

    def event_destroy(self, ev):
        if not self._closed:
            self.lib.ma_event_destroy(self.handle, ev)

    def clock_probe(self, milliseconds=20.0):
        """Sustained shader clock in GHz under a packed-FP32 load (ma_clock_probe)."""
        ghz = C.c_double()
        L.check(self.lib.ma_clock_probe(self.handle, float(milliseconds), C.byref(ghz)))
        return ghz.value

    def forget_host_arrays(self):
        """Drop every recorded host <-> device pair (Context.asdevice() uploads afresh); device memory held only by the
        pairs goes back to the pool."""
        self._resident.clear()

    def transfer_stats(self, reset=False):
        """(h2d_bytes, d2h_bytes) moved by this context's explicit host <-> device copies so far."""
        up, down = C.c_ulonglong(), C.c_ulonglong()
        L.check(self.lib.ma_ctx_transfer_stats(self.handle, C.byref(up), C.byref(down), int(bool(reset))))
        return up.value, down.value

    def close(self):
        if not self._closed:
            L.check(self.lib.ma_sync(self.handle))
            self.trim()
            # arrays that outlive the context: their HBM goes back to the driver now (they raise if used again)
            with self._host_lock:
                live, self._live = list(self._live), {}
                self._closed = True
            for p in live:
                self.lib.ma_free(self.handle, p)
            if getattr(self, "_zero_flags_ptr", None):
                self._zero_flags = None
                self.lib.ma_host_free(C.c_void_p(self._zero_flags_ptr))
                self._zero_flags_ptr = None
            if getattr(self, "_count_ptr", None):
                self._count_words = None
                self.lib.ma_host_free(C.c_void_p(self._count_ptr))
                self._count_ptr = None
            side, self._side = getattr(self, "_side", None), None
            if side is not None:
                side.close()
            self.lib.ma_ctx_destroy(self.handle)

    def side_context(self):
        """A second context on the same device, owned by this one (closed with it): an independent HIP stream, workspace and
        pools for work that may run beside this context's -- FeatureRegistrator puts the reference image's features of every
        level there while this one works through the moving image's coarse levels."""
        if getattr(self, "_side", None) is None:
            self._side = Context(self.device)
        return self._side

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- events / profiling --------------------------------------------------------------------
    def event(self):
        e = C.c_void_p()
        L.check(self.lib.ma_event_create(self.handle, C.byref(e)))
        return e

    def record(self, ev):
        L.check(self.lib.ma_event_record(self.handle, ev))

    def elapsed_ms(self, a, b):
        ms = C.c_float()
        L.check(self.lib.ma_event_elapsed_ms(self.handle, a, b, C.byref(ms)))
        return ms.value

    def profile(self, on=True):
        L.check(self.lib.ma_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        L.check(self.lib.ma_profile_reset(self.handle))

    def profile_get(self):
        out = {}
        for name, kid in L.KERNEL_IDS.items():
            ms, n, px = C.c_double(), C.c_longlong(), C.c_double()
            L.check(self.lib.ma_profile_get(self.handle, kid, C.byref(ms), C.byref(n), C.byref(px)))
            out[name] = {"ms": ms.value, "launches": n.value, "px": px.value}
        return out

    # -- primitives (device in, device out) ---------------------------------------------------
    def farneback(self, prev, nxt, winsize, iterations, tile=0, overlap=0, poly_n=1, poly_sigma=1.7, fused=False, levels=0):
        """cv2.calcOpticalFlowFarneback(prev, next, levels=0, GAUSSIAN) on the whole image (tile=0)
        or on TileFlowCalc's overlapping windows, stitched (flow_calc.py:59-98).  levels > 0: OpenCV's pyramid
        (pyr_scale 0.5) on the whole image (ma_farneback_levels)."""
        if prev.shape != nxt.shape or prev.ndim != 2:
            raise ValueError("prev/next must be 2-D arrays of the same shape")
        if levels > 0 and tile > 0:
            raise ValueError("levels > 0 runs on the whole image: tile must be 0")
        if prev.dtype != nxt.dtype:
            # cv2.calcOpticalFlowFarneback converts each input to float32 on its own (exact for integers): a mixed pair
            # is the float32 pair
            prev, nxt = self.to_f32(prev), self.to_f32(nxt)
        H, W = prev.shape
        flow = self.empty((H, W, 2), np.float32)
        if levels > 0:
            self._run(self.lib.ma_farneback_levels, prev.ptr, nxt.ptr, _dt(prev.dtype), H, W, int(levels), 0.5,
                      int(winsize), int(iterations), int(poly_n), float(poly_sigma),
                      L.MA_FB_MULADD_FUSED if fused else 0, flow.ptr)
            return flow
        self._run(self.lib.ma_farneback_tiled, prev.ptr, nxt.ptr, _dt(prev.dtype), H, W, int(tile),
                                            int(overlap), int(winsize), int(iterations), int(poly_n),
                                            float(poly_sigma), L.MA_FB_MULADD_FUSED if fused else 0, flow.ptr)
        return flow

    def farneback_debug(self, prev, nxt, winsize, iterations, poly_sigma=1.7, fused=False):
        H, W = prev.shape
        flow = self.empty((H, W, 2), np.float32)
        r0, r1, m0 = (self.empty((5, H, W), np.float32) for _ in range(3))
        self._run(self.lib.ma_farneback_debug, prev.ptr, nxt.ptr, _dt(prev.dtype), H, W, int(winsize),
                                            int(iterations), float(poly_sigma),
                                            L.MA_FB_MULADD_FUSED if fused else 0, flow.ptr, r0.ptr, r1.ptr, m0.ptr)
        return flow, r0, r1, m0

    def optflow_register(self, ref, mov, num_pyr_lvl=4, num_iterations=3, tile_size=1000, overlap=100,
                         use_full_res_img=False, use_dog=False, fb_flags=0, dog_flags=0):
        """OptFlowRegistrator.register() as one C call (ma_optflow_register): device images in, (flow DeviceArray,
        [(factor, (h, w), mi_after, mi_before, accepted), ...]) out.  The flow is enqueued, not synchronised."""
        if ref.shape != mov.shape or ref.dtype != mov.dtype or ref.ndim != 2:
            raise ValueError("ref/mov must be 2-D images of equal shape and dtype")
        H, W = ref.shape
        prm = L.MaParams(int(num_pyr_lvl), int(num_iterations), int(tile_size), int(overlap), int(bool(use_full_res_img)),
                         int(bool(use_dog)), int(fb_flags), int(dog_flags))
        nrep_max = max(int(num_pyr_lvl), 0) + 1
        reps = (L.MaLevelReport * nrep_max)()
        n = C.c_int(0)
        flow = self.empty((H, W, 2), np.float32)
        self._run(self.lib.ma_optflow_register, ref.ptr, mov.ptr, _dt(ref.dtype), H, W, C.byref(prm), flow.ptr, reps,
                  nrep_max, C.byref(n))
        return flow, [(r.factor, (r.h, r.w), r.mi_after, r.mi_before, bool(r.accepted)) for r in reps[:n.value]]

    def remap(self, src, map_xy, interpolation="linear"):
        """cv2.remap(src, map_xy, None, interpolation): "nearest", "linear", "cubic", "lanczos4" or cv2's codes 0, 1, 2, 4
        (include/microaligner_interp.h)."""
        interp = interp_code(interpolation)
        cn = 1 if src.ndim == 2 else src.shape[2]
        sh, sw = src.shape[:2]
        dh, dw = map_xy.shape[:2]
        if map_xy.dtype != np.float32 or map_xy.ndim != 3 or map_xy.shape[2] != 2:
            raise ValueError("map must be (h, w, 2) float32")
        dst = self.empty((dh, dw) if src.ndim == 2 else (dh, dw, cn), src.dtype)
        if interp == L.MA_INTER_LINEAR:
            self._run(self.lib.ma_remap_bilinear, src.ptr, _dt(src.dtype), cn, sh, sw, map_xy.ptr, dh, dw,
                                               dst.ptr)
        else:
            self._run(self.lib.ma_remap_interp, src.ptr, _dt(src.dtype), cn, sh, sw, map_xy.ptr, dh, dw, dst.ptr, interp)
        return dst

    def warp(self, img, flow, tile, overlap, minmax=False, flow_cells=False, interpolation="linear"):
        """Warper.warp() (warper.py:37-53).  minmax=True also leaves the output's (min, max) on the device
        (out.minmax) for a following dog_u8; flow_cells=True the per-cell maxima of `flow` (flow.cellkeys) for a
        following merge_flows (only where the tiling has cells: tile > 2*overlap > 0).  interpolation: as remap(); the
        by-products belong to the linear warp of register() and are not offered with the other modes."""
        interp = interp_code(interpolation)
        H, W = img.shape
        if flow.shape != (H, W, 2) or flow.dtype != np.float32:
            raise ValueError(f"flow must be float32 of shape {(H, W, 2)}, got {flow.dtype} {flow.shape}")
        if interp != L.MA_INTER_LINEAR:
            if minmax or flow_cells:
                raise ValueError("minmax / flow_cells are by-products of the linear warp only")
            out = self.empty((H, W), img.dtype)
            self._run(self.lib.ma_warp_tiled_interp, img.ptr, _dt(img.dtype), H, W, flow.ptr, int(tile), int(overlap),
                      out.ptr, interp)
            return out
        out = self.empty((H, W), img.dtype)
        if flow_cells and tile > 2 * overlap > 0:
            ncell = (2 * -(-W // tile) + 1) * (2 * -(-H // tile) + 1)
            keys = self._raw(L.MA_FLOW_CELL_REPLICAS * ncell * 4)
            if minmax:
                out.minmax = self.empty((2,), np.float32)
            self._run(self.lib.ma_warp_tiled_flowcells, img.ptr, _dt(img.dtype), H, W, flow.ptr, int(tile), int(overlap),
                      out.ptr, out.minmax.ptr if minmax else None, keys.ptr)
            flow.cellkeys = (int(tile), int(overlap), keys)
            return out
        if minmax:
            out.minmax = self.empty((2,), np.float32)
            self._run(self.lib.ma_warp_tiled_minmax, img.ptr, _dt(img.dtype), H, W, flow.ptr, int(tile),
                                                  int(overlap), out.ptr, out.minmax.ptr)
        else:
            self._run(self.lib.ma_warp_tiled, img.ptr, _dt(img.dtype), H, W, flow.ptr, int(tile),
                                           int(overlap), out.ptr)
        return out

    @staticmethod
    def _page_pointers(pages, out, out_shape, out_what):
        """The results of a page warp (allocated if `out` is None, checked otherwise) and the two pointer arrays the
        page-warp entry points take: (out, n, src, dst)."""
        if out is None:
            out = [np.empty(out_shape, pages[0].dtype) for _ in pages]
        if len(out) != len(pages) or any(o.shape != out_shape or o.dtype != pages[0].dtype or not o.flags.c_contiguous
                                         or not o.flags.writeable for o in out):
            raise ValueError(f"out must hold one writable C-contiguous array of {out_what} per page")
        n = len(pages)
        return out, n, (C.c_void_p * n)(*[p.ctypes.data for p in pages]), (C.c_void_p * n)(*[o.ctypes.data for o in out])

    def warp_pages(self, pages, flow, tile, overlap, out=None, interpolation="linear"):
        """warp_and_save_pages (__main__.py:288-302): warp every HOST page with one device-resident flow.
        pages: sequence of equal-shape C-contiguous numpy arrays; out: optional sequence of writable arrays of the
        same shape/dtype (e.g. memmap rows), allocated if None; interpolation: as remap().  Returns `out`."""
        interp = interp_code(interpolation)
        pages = [np.ascontiguousarray(p) for p in pages]
        if not pages:
            return []
        H, W = pages[0].shape
        dt = _dt(pages[0].dtype)
        if any(p.shape != (H, W) or p.dtype != pages[0].dtype for p in pages):
            raise ValueError("all pages must have the same shape and dtype")
        if flow.shape != (H, W, 2) or flow.dtype != np.float32:
            raise ValueError(f"flow must be float32 of shape {(H, W, 2)}, got {flow.dtype} {flow.shape}")
        if getattr(flow, "ctx", self) is not self:
            raise ValueError("flow belongs to another context")
        out, n, src, dst = self._page_pointers(pages, out, (H, W), "the page shape/dtype")
        if interp == L.MA_INTER_LINEAR:
            self._run(self.lib.ma_warp_pages_host, src, dst, n, dt, H, W, flow.ptr, int(tile), int(overlap))
        else:
            self._run(self.lib.ma_warp_pages_host_interp, src, dst, n, dt, H, W, flow.ptr, int(tile), int(overlap), interp)
        return out

    def warp_affine_flow(self, img, flow, tmat, interpolation="linear"):
        """One resampling of `img` (h, w) through the 2x3 matrix `tmat` and the (H, W, 2) `flow` (h <= H, w <= W):
        cv2.remap(pad_to_shape(img, (H, W)), float32(M.(p - flow(p))), interpolation) with M = pinv([tmat; 0 0 1]), the
        whole image at once (no tile windows), integer coordinates not saturated to 16 bits
        (include/microaligner_compose.h).  What transform_img_with_tmat followed by Warper.warp() approximates with two
        resamplings.  Returns a DeviceArray (H, W)."""
        interp, m, left, top = affine_flow_params(img.shape, img.dtype, flow.shape, flow.dtype, tmat, interpolation)
        img, flow = self.asdevice(img), self.asdevice(flow)
        (h, w), (H, W) = img.shape, flow.shape[:2]
        out = self.empty((H, W), img.dtype)
        self._run(self.lib.ma_warp_affine_flow, img.ptr, _dt(img.dtype), h, w, left, top, flow.ptr, H, W,
                  (C.c_double * 6)(*[float(v) for v in m]), out.ptr, interp)
        return out

    def warp_affine_flow_pages(self, pages, flow, tmat, out=None, interpolation="linear"):
        """warp_affine_flow() for many HOST pages (h, w) with one device-resident flow (H, W, 2): the page-warp driver of
        include/microaligner_compose.h uploads page i + 1 while page i is warped and downloads the results in bands.
        out: optional sequence of writable C-contiguous (H, W) arrays (e.g. memmap rows), allocated if None.  Returns `out`."""
        pages = [np.ascontiguousarray(p) for p in pages]
        if not pages:
            return []
        interp, m, left, top = affine_flow_params(pages[0].shape, pages[0].dtype, flow.shape, flow.dtype, tmat,
                                                  interpolation)
        (h, w), (H, W) = pages[0].shape, flow.shape[:2]
        if any(p.shape != (h, w) or p.dtype != pages[0].dtype for p in pages):
            raise ValueError("all pages must have the same shape and dtype")
        if getattr(flow, "ctx", self) is not self:
            raise ValueError("flow belongs to another context")
        flow = self.asdevice(flow)
        out, n, src, dst = self._page_pointers(pages, out, (H, W), "the flow's (H, W) and the page dtype")
        self._run(self.lib.ma_warp_affine_flow_pages_host, src, dst, n, _dt(pages[0].dtype), h, w, left, top, flow.ptr,
                  H, W, (C.c_double * 6)(*[float(v) for v in m]), interp)
        return out

    # grid flows (include/microaligner_flowgrid.h) -------------------------------------------------------------------------
    def flow_grid_sample(self, flow, stride):
        """The FlowGrid (device nodes) of a device-resident (H, W, 2) float32 flow at `stride`: point sampling."""
        H, W = _check_flow(flow)
        stride = _check_stride(stride)
        nodes = self.empty((grid_nodes(H, stride), grid_nodes(W, stride), 2), np.float32)
        self._run(self.lib.ma_flow_grid_sample, flow.ptr, H, W, stride, nodes.ptr)
        return FlowGrid(nodes, stride, (H, W))

    def _grid_nodes(self, grid, side_max=1 << 24):
        """the device nodes of a FlowGrid of this context"""
        if not isinstance(grid, FlowGrid):
            raise ValueError(f"expected a FlowGrid, got {type(grid).__name__}")
        if max(grid.shape) > side_max:
            raise ValueError(f"flow sides must be at most {side_max}, got {grid.shape}")
        if getattr(grid.nodes, "ctx", self) is not self:
            raise ValueError("the grid's nodes belong to another context")
        return self.asdevice(grid.nodes)

    def flow_grid_expand(self, grid):
        """The dense flow of a FlowGrid as a DeviceArray (H, W, 2)."""
        nodes = self._grid_nodes(grid)
        H, W = grid.shape
        out = self.empty((H, W, 2), np.float32)
        self._run(self.lib.ma_flow_grid_expand, nodes.ptr, H, W, grid.stride, out.ptr)
        return out

    def flow_grid_error(self, flow, grid, cell_h, cell_w, tol):
        """Per cell of the (cell_h, cell_w) grid, what `grid` loses against the device-resident `flow`:
        (max_err float32, above int64, invalid int64), each (gy, gx) on the host."""
        H, W = _check_flow(flow)
        nodes = self._grid_nodes(grid)
        if grid.shape != (H, W):
            raise ValueError(f"the grid belongs to a flow of shape {grid.shape}, got {(H, W)}")
        gy, gx = self._cell_grid_shape(H, W, min(int(cell_h), H), min(int(cell_w), W))
        max_err = np.empty((gy, gx), np.float32)
        above, invalid = np.empty((gy, gx), np.int64), np.empty((gy, gx), np.int64)
        pl = C.POINTER(C.c_longlong)
        self._run(self.lib.ma_flow_grid_error, flow.ptr, nodes.ptr, H, W, grid.stride, int(cell_h), int(cell_w), float(tol),
                  max_err.ctypes.data_as(C.POINTER(C.c_float)), above.ctypes.data_as(pl), invalid.ctypes.data_as(pl))
        return max_err, above, invalid

    def warp_affine_grid(self, img, grid, tmat=None, interpolation="linear"):
        """warp_affine_flow() with the flow given by a FlowGrid, evaluated from its nodes inside the warp kernel: the
        result is warp_affine_flow(img, grid.expand(), tmat) bit for bit, and the dense flow is never built.  tmat None: the
        identity and no padding.  Returns a DeviceArray (H, W)."""
        interp, m, left, top = affine_grid_params(img.shape, img.dtype, grid, tmat, interpolation)
        img, nodes = self.asdevice(img), self._grid_nodes(grid, 1 << 30)
        (h, w), (H, W) = img.shape, grid.shape
        out = self.empty((H, W), img.dtype)
        self._run(self.lib.ma_warp_affine_grid, img.ptr, _dt(img.dtype), h, w, left, top, nodes.ptr, H, W, grid.stride,
                  (C.c_double * 6)(*[float(v) for v in m]), out.ptr, interp)
        return out

    def warp_affine_grid_pages(self, pages, grid, tmat=None, out=None, interpolation="linear"):
        """warp_affine_grid() for many HOST pages (h, w) through the page-warp driver of warp_affine_flow_pages(), with
        the same band plan.  Returns `out`."""
        pages = [np.ascontiguousarray(p) for p in pages]
        if not pages:
            return []
        interp, m, left, top = affine_grid_params(pages[0].shape, pages[0].dtype, grid, tmat, interpolation)
        (h, w), (H, W) = pages[0].shape, grid.shape
        if any(p.shape != (h, w) or p.dtype != pages[0].dtype for p in pages):
            raise ValueError("all pages must have the same shape and dtype")
        nodes = self._grid_nodes(grid, 1 << 30)
        out, n, src, dst = self._page_pointers(pages, out, (H, W), "the flow's (H, W) and the page dtype")
        self._run(self.lib.ma_warp_affine_grid_pages_host, src, dst, n, _dt(pages[0].dtype), h, w, left, top, nodes.ptr,
                  H, W, grid.stride, (C.c_double * 6)(*[float(v) for v in m]), interp)
        return out

    def merge_flows(self, flow1, flow2, tile, overlap):
        """_merge_flow_in_tiles (optflow_registrator.py:217-233)."""
        if flow1.shape != flow2.shape:
            raise ValueError("flows must have the same shape")
        H, W = flow1.shape[:2]
        out = self.empty((H, W, 2), np.float32)
        k1, k2 = flow1.cellkeys, flow2.cellkeys
        if k1 is not None and k2 is not None and k1[:2] == k2[:2] == (int(tile), int(overlap)):
            # both flows went through a warp that folded their cell maxima: no pass over the flows for the .max() tests
            self._run(self.lib.ma_merge_flows_tiled_cells, flow1.ptr, flow2.ptr, H, W, int(tile), int(overlap),
                      k1[2].ptr, k2[2].ptr, out.ptr)
        else:
            self._run(self.lib.ma_merge_flows_tiled, flow1.ptr, flow2.ptr, H, W, int(tile), int(overlap), out.ptr)
        return out

    def compose_flows(self, first, second):
        """The flow of "warp by first, then warp the result by second": second + first sampled at (p - second), whole
        image, replicate border (include/microaligner_flowcompose.h).  Device arrays in, a new device array out."""
        for name, f in (("first", first), ("second", second)):
            if f.dtype != np.float32 or len(f.shape) != 3 or f.shape[2] != 2:
                raise ValueError(f"{name} must be an (H, W, 2) float32 flow, got {tuple(f.shape)} {f.dtype}")
        if tuple(first.shape) != tuple(second.shape):
            raise ValueError(f"flows must have the same shape, got {tuple(first.shape)} and {tuple(second.shape)}")
        H, W = first.shape[:2]
        if not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
            raise ValueError(f"flow sides must be in [1, 2^24], got {(H, W)}")
        out = self.empty((H, W, 2), np.float32)
        self._run(self.lib.ma_compose_flows, first.ptr, second.ptr, H, W, out.ptr)
        return out

    def invert_flow(self, flow, max_iter=50, tol=1e-3, return_info=False):
        """The inverse g of a flow f: g(q) = -f(q - g(q)), so that compose_flows(f, g) ~ 0, by a fixed-point iteration per
        pixel in one kernel (include/microaligner_flowinvert.h).  A device array in, a new device array out; with
        return_info an InvertInfo(not_converged, residual as a device array) beside it, at the cost of a synchronisation."""
        H, W, max_iter, tol = invert_flow_params(flow, max_iter, tol)
        out = self.empty((H, W, 2), np.float32)
        if not return_info:
            self._run(self.lib.ma_invert_flow, flow.ptr, H, W, max_iter, tol, out.ptr, None, None)
            return out
        residual, count = self.empty((H, W), np.float32), C.c_longlong(0)
        self._run(self.lib.ma_invert_flow, flow.ptr, H, W, max_iter, tol, out.ptr, residual.ptr, C.byref(count))
        return out, InvertInfo(int(count.value), residual)

    def _flow_out(self, out, H, W):
        """the `out` of a call that may write its flow in place: a new (H, W, 2) float32 array for None"""
        if out is None:
            return self.empty((H, W, 2), np.float32)
        if not isinstance(out, DeviceArray) or out.dtype != np.float32 or out.shape != (H, W, 2):
            raise ValueError(f"out must be a float32 DeviceArray of shape {(H, W, 2)}")
        return out

    def _class_counts(self, H, W, ch, cw, classes):
        """the (gy, gx, classes) int64 array of per-cell counts and its pointer for the C entry; None twice without cells"""
        if ch is None:
            return None, None
        counts = np.empty(self._cell_grid_shape(H, W, min(ch, H), min(cw, W)) + (classes,), np.int64)
        return counts, counts.ctypes.data_as(C.POINTER(C.c_longlong))

    def smooth_flow(self, flow, taps, weight=None, cell_size=None, where="all", min_support=0.0, return_info=False, out=None):
        """The weighted smoothing of a flow with the symmetric kernel taps t[0 .. r] (include/microaligner_flowsmooth.h): a
        row pass and a column pass over w*u, w*v, w, the divide, and for where="blend" the feathering back into the
        untouched flow.  Device arrays in (weight: None, an (H, W) float32 or uint8 array, or with cell_size a (gy, gx)
        float32 map), a new device array out; `out` may name the array to write instead, `flow` itself included.  With
        return_info a SmoothInfo(unsupported) beside it, at the cost of a synchronisation."""
        H, W, taps, r, kind, ch, cw, mode, ms = smooth_flow_params(flow, taps, weight, cell_size, where, min_support)
        out = self._flow_out(out, H, W)
        count = C.c_longlong(0)
        self._run(self.lib.ma_smooth_flow, flow.ptr, H, W, taps.ctypes.data_as(C.POINTER(C.c_float)), r,
                  None if weight is None else weight.ptr, kind, ch, cw, mode, ms, out.ptr,
                  C.byref(count) if return_info else None)
        return (out, SmoothInfo(int(count.value))) if return_info else out

    def fold_mask(self, flow, margin=2, return_info=False):
        """keep (H, W) uint8: 0 within `margin` pixels (Chebyshev) of a pixel where the flow folds (det J <= 0) or is not
        finite, else 1 (include/microaligner_flowsmooth.h).  A device array in, a new device array out; with return_info a
        FoldInfo(folded, invalid, dropped) beside it, at the cost of a synchronisation."""
        H, W, margin = fold_mask_params(flow, margin)
        keep = self.empty((H, W), np.uint8)
        counts = (C.c_longlong * 3)()
        self._run(self.lib.ma_flow_fold_mask, flow.ptr, H, W, margin, keep.ptr, counts if return_info else None)
        return (keep, FoldInfo(*(int(v) for v in counts))) if return_info else keep

    def median_flow(self, flow, radius=2, weight=None, cell_size=None, where="all", thresh=None, return_info=False, out=None,
                    keep=False, generic=False):
        """The median filter of a flow over (2 radius + 1)^2 windows and its outlier mask
        (include/microaligner_flowmedian.h), in one kernel.  Device arrays in (weight: None, an (H, W) float32 or uint8
        array, or with cell_size a (gy, gx) float32 map; read as a mask), new device arrays out.
        out: None -- a new (H, W, 2) array; a DeviceArray to write instead (never `flow` itself: a median reads its
        neighbours); False -- no flow is made (keep only).  keep: False -- no mask; True -- a new (H, W) uint8 array; or a
        DeviceArray to write.  generic: take the kernel that serves every radius, also where radius <= 3 (same bits).
        Returns what was made, in the order out, keep, and with return_info a MedianInfo(outliers, dropped, unsupported)
        at the cost of a synchronisation: one object alone, or a tuple of them."""
        H, W, r, kind, ch, cw, mode, th, flags = median_flow_params(flow, radius, weight, cell_size, where, thresh, generic)
        if out is flow:
            raise ValueError("out must not be the flow: a median reads its neighbours")
        if out is False and keep is False:
            raise ValueError("nothing to make: out=False needs a keep")
        if out is not None and out is not False and \
                (not isinstance(out, DeviceArray) or out.dtype != np.float32 or out.shape != (H, W, 2)):
            raise ValueError(f"out must be a float32 DeviceArray of shape {(H, W, 2)}, None or False")
        if not isinstance(keep, bool) and \
                (not isinstance(keep, DeviceArray) or keep.dtype != np.uint8 or keep.shape != (H, W)):
            raise ValueError(f"keep must be a uint8 DeviceArray of shape {(H, W)} or a bool")
        if out is None:
            out = self.empty((H, W, 2), np.float32)
        if keep is True:
            keep = self.empty((H, W), np.uint8)
        counts = (C.c_longlong * 3)()
        self._run(self.lib.ma_median_flow, flow.ptr, H, W, r, None if weight is None else weight.ptr, kind, ch, cw, mode, th,
                  flags, None if out is False else out.ptr, None if keep is False else keep.ptr,
                  counts if return_info else None)
        res = [a for a in (out, keep) if a is not False]
        if return_info:
            res.append(MedianInfo(*(int(v) for v in counts)))
        return res[0] if len(res) == 1 else tuple(res)

    def fill_flow(self, flow, weight=None, cell_size=None, return_info=False, out=None):
        """The push-pull fill of a flow (include/microaligner_flowfill.h): a weighted pyramid pulled to 1 x 1 and pushed
        back, pixels of weight >= 1 coming back bit for bit.  Device arrays in (weight: None, an (H, W) float32 or uint8
        array, or with cell_size a (gy, gx) float32 map), a new device array out; `out` may name the array to write instead,
        `flow` itself included, never the weight.  With return_info a FillInfo(dropped, blended, unsupported, levels)
        beside it, at the cost of a synchronisation."""
        H, W, kind, ch, cw, levels = fill_flow_params(flow, weight, cell_size)
        if out is not None and out is weight:
            raise ValueError("out must not be the weight")
        out = self._flow_out(out, H, W)
        counts = (C.c_longlong * 3)()
        self._run(self.lib.ma_fill_flow, flow.ptr, H, W, None if weight is None else weight.ptr, kind, ch, cw, out.ptr,
                  counts if return_info else None)
        return (out, FillInfo(*(int(v) for v in counts), levels)) if return_info else out

    def texture_maps(self, img, taps, floor=None, cell_size=None, want=("lam_min", "lam_max")):
        """The texture support maps of an (H, W) uint8, uint16 or float32 device image with the symmetric kernel taps
        t[0 .. r] (include/microaligner_texture.h): the eigenvalues of its smoothed structure tensor, and with `floor` (in
        squared grey levels) the weight lam_min / (lam_min + floor) and, with cell_size, the per-cell counts of textured,
        edge and flat pixels.  -> a dict of the planes named in `want` ((H, W) float32 device arrays) and, with cell_size,
        "counts": a (gy, gx, 3) int64 numpy array, at the cost of a synchronisation."""
        H, W, dtype, taps, r, floor, ch, cw, want = texture_maps_params(img, taps, floor, cell_size, want)
        out = {n: self.empty((H, W), np.float32) for n in want}
        ptr = {n: (out[n].ptr if n in out else None) for n in TEXTURE_PLANES}
        counts, counts_ptr = self._class_counts(H, W, ch, cw, L.MA_TEXTURE_CLASSES)
        self._run(self.lib.ma_texture_maps, img.ptr, dtype, H, W, taps.ctypes.data_as(C.POINTER(C.c_float)), r,
                  0.0 if floor is None else floor, ptr["lam_min"], ptr["lam_max"], ptr["weight"], ch or 0, cw or 0, counts_ptr)
        if counts is not None:
            out["counts"] = counts
        return out

    def local_correlation(self, ref, img, taps, floor, center=(0.0, 0.0), weight=None, lo=0.25, hi=0.75, min_support=0.0,
                          cell_size=None, want=("score",)):
        """The local correlation maps of an (H, W) uint8, uint16 or float32 device image `ref` and an (H, W) float32 device
        image `img` on its grid, with the symmetric kernel taps t[0 .. r] (include/microaligner_localcorr.h): the windowed
        ZNCC of ref - center[0] and img - center[1] with `floor` (in squared grey levels) under both variances, NaN where
        the window's weight is not above min_support; the weight that is 0 below `lo`, 1 from `hi` on and linear between;
        and, with cell_size, the per-cell counts of agreeing, disagreeing, flat and unsupported pixels.  weight: None, an
        (H, W) float32 map or uint8 mask.  -> a dict of the planes named in `want` ((H, W) float32 device arrays) and, with
        cell_size, "counts": a (gy, gx, 4) int64 numpy array, at the cost of a synchronisation."""
        H, W, rdt, taps, r, (ca, cb), floor, kind, ms, lo, hi, ch, cw, want = local_correlation_params(
            ref, img, taps, floor, center, weight, lo, hi, min_support, cell_size, want)
        out = {n: self.empty((H, W), np.float32) for n in want}
        ptr = {n: (out[n].ptr if n in out else None) for n in LOCALCORR_PLANES}
        counts, counts_ptr = self._class_counts(H, W, ch, cw, L.MA_LOCALCORR_CLASSES)
        self._run(self.lib.ma_local_correlation, ref.ptr, rdt, img.ptr, H, W, taps.ctypes.data_as(C.POINTER(C.c_float)), r,
                  ca, cb, floor, None if weight is None else weight.ptr, kind, ms, lo, hi, ptr["score"], ptr["weight"],
                  ch or 0, cw or 0, counts_ptr)
        if counts is not None:
            out["counts"] = counts
        return out

    def normalize_local(self, img, taps, floor, clip=4.0, weight=None, min_support=0.0, want=("u8",), return_info=False):
        """The local contrast normalisation of an (H, W) uint8, uint16 or float32 device image with the symmetric kernel
        taps t[0 .. r] (include/microaligner_localnorm.h): z = (x - mu) / sqrt(v + floor) with the windowed mean mu and the
        windowed variance v about it, `floor` in squared grey levels; "f32": z clipped to +-clip, "u8": z * 127 / clip + 128
        rounded into 0 .. 255.  Pixels that are dropped (not finite, or no weight) or whose window's weight is not above
        min_support give 0.0 / 128.  weight: None, an (H, W) float32 map or uint8 mask.  -> a dict of the planes named in
        `want` ((H, W) device arrays); with return_info (that dict, LocalNormInfo(dropped, unsupported, flat, clipped)),
        at the cost of a synchronisation."""
        H, W, dtype, taps, r, floor, clip, kind, ms, want = local_norm_params(img, taps, floor, clip, weight, min_support, want)
        out = {n: self.empty((H, W), np.uint8 if n == "u8" else np.float32) for n in want}
        ptr = {n: (out[n].ptr if n in out else None) for n in LOCALNORM_PLANES}
        counts = (C.c_longlong * L.MA_LOCALNORM_COUNTS)()
        self._run(self.lib.ma_normalize_local, img.ptr, dtype, H, W, taps.ctypes.data_as(C.POINTER(C.c_float)), r, floor, clip,
                  None if weight is None else weight.ptr, kind, ms, ptr["f32"], ptr["u8"], counts if return_info else None)
        return (out, LocalNormInfo(*(int(v) for v in counts))) if return_info else out

    def morphology(self, img, op, radius, out=None):
        """The flat grey morphology of an (H, W) uint8, uint16 or float32 device image over the rectangle of
        (2 ry + 1) x (2 rx + 1) pixels, radius = r or (ry, rx), each 0 .. 255 (include/microaligner_morphology.h): op
        "erode" / "dilate" the smallest / largest value of the window cut at the border, "open" = dilate(erode),
        "close" = erode(dilate), "tophat" = img - open, "blackhat" = close - img.  Exact: every result but a hat's is one of
        the input values; float32 NaNs take no part in a window.  A new device array of img's dtype out; `out` may name the
        array to write instead, `img` itself included."""
        H, W, dtype, code, ry, rx = morphology_params(img, op, radius)
        if out is None:
            out = self.empty((H, W), img.dtype)
        elif not isinstance(out, DeviceArray) or out.dtype != img.dtype or out.shape != (H, W):
            raise ValueError(f"out must be a {np.dtype(img.dtype)} DeviceArray of shape {(H, W)}")
        self._run(self.lib.ma_morphology, img.ptr, dtype, H, W, code, ry, rx, out.ptr)
        return out

    # connected components (include/microaligner_components.h) -----------------------------------------------------------
    def components_asdevice(self, img):
        """An image of the connected components on the device: a DeviceArray passes through, a numpy bool array is taken as
        uint8, and a uint8, uint16 or int32 array is uploaded (asdevice() holds to the three image dtypes)."""
        if isinstance(img, DeviceArray):
            return img
        arr = np.ascontiguousarray(img)
        if arr.dtype == np.bool_:
            arr = arr.view(np.uint8)
        if arr.dtype != np.int32:
            return self.asdevice(arr)
        d = self.empty(arr.shape, np.int32)
        if arr.nbytes:
            L.check(self.lib.ma_memcpy_h2d(self.handle, d.ptr, arr.ctypes.data, arr.nbytes))
        return d

    def _cc_out(self, img, out, dtype):
        H, W = img.shape
        if out is None:
            return self.empty((H, W), dtype)
        if not isinstance(out, DeviceArray) or out.dtype != np.dtype(dtype) or out.shape != (H, W):
            raise ValueError(f"out must be a {np.dtype(dtype)} DeviceArray of shape {(H, W)}")
        return out

    def label_components(self, img, connectivity=1, by_value=False, out=None):
        """The connected components of an (H, W) uint8, uint16 or int32 device image (include/microaligner_components.h) ->
        (labels, n): an int32 device array, 0 for background and k = 1 .. n for the component that is the k-th by its
        smallest linear index y * W + x (scipy.ndimage.label's numbering), and the number of components.  A pixel is
        foreground when it is not 0; connectivity 1 joins the 4 edge neighbours, 2 the 8 neighbours; by_value joins
        neighbours only where their values are equal.  `out` may name the int32 array to write, but not `img`.  Waits for
        the stream: n is a host value."""
        H, W, dtype, flags = components_params(img, connectivity, by_value)
        out = self._cc_out(img, out, np.int32)
        if out is img:
            raise ValueError("out must not be img")
        n = C.c_longlong(-1)
        self._run(self.lib.ma_cc_label, img.ptr, dtype, H, W, flags, out.ptr, C.byref(n))
        return out, int(n.value)

    def component_stats(self, labels, n):
        """The areas and boxes of an (H, W) int32 device image of labels 0 .. n -> (areas, bboxes): device arrays of
        (n + 1,) int64, areas[0] the background's, and (n + 1, 4) int32, y0, x0, y1, x1 with the ends exclusive, row 0 and
        the rows of absent labels zeros.  Stream ordered."""
        H, W, dtype, _ = components_params(labels)
        if dtype != L.MA_CC_I32:
            raise ValueError(f"labels must be int32, got {labels.dtype}")
        if not _is_int(n) or not 0 <= n <= L.MA_CC_MAX_PIXELS - 1:
            raise ValueError(f"n must be an int in [0, 2^31 - 2], got {n!r}")
        areas, bboxes = self.empty((n + 1,), np.int64), self.empty((n + 1, 4), np.int32)
        self._run(self.lib.ma_cc_stats, labels.ptr, H, W, int(n), areas.ptr, bboxes.ptr)
        return areas, bboxes

    def remove_small_objects(self, img, min_size, connectivity=1, by_value=False, out=None):
        """img with every foreground pixel set to 0 whose component (label_components' components) has fewer than min_size
        pixels; every other pixel bit for bit.  A new device array of img's dtype; `out` may name the array to write, `img`
        itself included.  Stream ordered."""
        H, W, dtype, flags, min_size = remove_small_params(img, min_size, connectivity, by_value)
        out = self._cc_out(img, out, img.dtype)
        if min_size > H * W:                        # no component is that large: every pixel becomes 0
            L.check(self.lib.ma_memset(self.handle, out.ptr, 0, out.nbytes))
        elif min_size <= 1:                         # every component is that large
            if out is not img:
                L.check(self.lib.ma_memcpy_d2d(self.handle, out.ptr, img.ptr, img.nbytes))
        else:
            self._run(self.lib.ma_cc_filter, img.ptr, dtype, H, W, flags, min_size, L.MA_CC_MAX_PIXELS, 0, out.ptr)
        return out

    def fill_holes(self, img, max_size=None, connectivity=1, value=1, out=None):
        """img with every enclosed hole set to `value`: a hole is a component of the pixels that are 0, joined under
        `connectivity`, that has no pixel in the first or last row or column and, with max_size, at most max_size pixels.
        Every other pixel bit for bit.  A new device array of img's dtype; `out` may name the array to write, `img` itself
        included.  Stream ordered."""
        H, W, dtype, flags, max_area, value = fill_holes_params(img, max_size, connectivity, value)
        out = self._cc_out(img, out, img.dtype)
        self._run(self.lib.ma_cc_filter, img.ptr, dtype, H, W, flags, 0, max_area, value, out.ptr)
        return out

    def flow_refine_step(self, ref, warped, flow, taps, floor, weight=None, max_step=1.0, return_info=False, out=None):
        """One regularised Lucas-Kanade step of `flow` (include/microaligner_flowrefine.h): the 2 x 2 system of the
        structure tensor of `warped` -- the float32 moving image resampled by `flow` -- smoothed with the symmetric kernel
        taps t[0 .. r], plus `floor` on its diagonal, against the smoothed products of the gradients and warped - ref; the
        solution, each component clamped to +-max_step, is added to the flow.  Device arrays in (ref: (H, W) uint8, uint16
        or float32; weight: None, an (H, W) float32 map or uint8 mask), a new device array out; `out` may name the array to
        write instead, `flow` itself included.  With return_info a RefineStepInfo(step_max, clamped, invalid) beside it, at
        the cost of a synchronisation."""
        H, W, rdt, taps, r, floor, kind, max_step = flow_refine_step_params(ref, warped, flow, taps, floor, weight, max_step)
        out = self._flow_out(out, H, W)
        stats = (C.c_longlong * L.MA_REFINE_STATS)()
        self._run(self.lib.ma_flow_refine_step, ref.ptr, rdt, warped.ptr, H, W, taps.ctypes.data_as(C.POINTER(C.c_float)), r,
                  floor, None if weight is None else weight.ptr, kind, max_step, flow.ptr, out.ptr,
                  stats if return_info else None)
        if not return_info:
            return out
        step_max = float(np.array([stats[2]], np.uint32).view(np.float32)[0])
        return out, RefineStepInfo(step_max, int(stats[1]), int(stats[0]))

    def flow_affine_moments(self, flow, weight=None, cell_size=None, prior=None, clip=None):
        """The 14 weighted sums and 4 counts from which an affine fit of a flow is solved, per cell of the cell_size grid
        (None: one cell, the whole image), about the image's centre (include/microaligner_flowaffine.h).  Device arrays in
        (weight: None, an (H, W) float32 or uint8 array, or with cell_size a (gy, gx) float32 map); prior / clip: a 2 x 3
        matrix in the centred frame and the residual in px beyond which a pixel is left out.  -> (sums (gy, gx, 14)
        float64, counts (gy, gx, 4) int64 of used, invalid, unweighted, trimmed).  Synchronises."""
        H, W, kind, ch, cw, pr, clip = flow_affine_moments_params(flow, weight, cell_size, prior, clip)
        gy, gx = self._cell_grid_shape(H, W, min(ch, H), min(cw, W))
        sums = np.empty((gy, gx, L.MA_FLOW_AFFINE_SUMS), np.float64)
        counts = np.empty((gy, gx, L.MA_FLOW_AFFINE_COUNTS), np.int64)
        self._run(self.lib.ma_flow_affine_moments, flow.ptr, H, W, None if weight is None else weight.ptr, kind, ch, cw,
                  None if pr is None else pr.ctypes.data_as(C.POINTER(C.c_double)), clip,
                  sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_longlong)))
        return sums, counts

    def flow_affine_apply(self, flow, mat, out=None):
        """apply(flow, A)(p) = p - A (p - flow(p)) in float64, rounded to float32 (include/microaligner_flowaffine.h): the
        flow relative to the 2 x 3 matrix A (split), or with A = inv([tmat; 0 0 1]) the total flow of a matrix and a flow
        relative to it (join).  A device array in, a new device array out; `out` may name the array to write instead,
        `flow` itself included."""
        H, W, a = flow_affine_apply_params(flow, mat)
        out = self._flow_out(out, H, W)
        self._run(self.lib.ma_flow_affine_apply, flow.ptr, H, W, a.ctypes.data_as(C.POINTER(C.c_double)), out.ptr)
        return out

    def direct_affine_moments(self, ref, mov, M, gain=1.0, bias=0.0, weight=None, clip=None):
        """The 31 weighted sums and 5 counts of one Gauss-Newton pass of the intensity-based affine alignment
        (include/microaligner_direct.h): the reference against gain * mov(M p) + bias, mov sampled bilinearly, about the
        image's centre.  Device arrays in (ref, mov: (H, W) uint8, uint16 or float32; weight: None, an (H, W) float32 map
        or uint8 mask); M: 2 x 3, reference pixels to moving-image pixels; clip: the residual in grey levels beyond which a
        pixel is left out.  -> (sums (31,) float64, counts (5,) int64 of used, outside, invalid, unweighted, trimmed).
        Synchronises."""
        H, W, rdt, mdt, m, gain, bias, kind, clip = direct_affine_moments_params(ref, mov, M, gain, bias, weight, clip)
        sums = np.empty((L.MA_DIRECT_AFFINE_SUMS,), np.float64)
        counts = np.empty((L.MA_DIRECT_AFFINE_COUNTS,), np.int64)
        self._run(self.lib.ma_direct_affine_moments, ref.ptr, rdt, mov.ptr, mdt, H, W, m.ctypes.data_as(C.POINTER(C.c_double)),
                  gain, bias, None if weight is None else weight.ptr, kind, clip,
                  sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_longlong)))
        return sums, counts

    def mask_weight(self, mask):
        """A uint8 device mask as the float32 map of the same weights, nonzero = 1.0 (include/microaligner_direct.h): what
        the pyramid of a mask is built from.  Stream ordered."""
        if not isinstance(mask, DeviceArray) or mask.dtype != np.uint8 or mask.size < 1:
            raise ValueError("mask must be a non-empty uint8 DeviceArray")
        out = self.empty(mask.shape, np.float32)
        self._run(self.lib.ma_direct_mask_weight, mask.ptr, mask.size, out.ptr)
        return out

    def transform_points(self, points, flow, direction, tmat=None, image_shape=None, max_iter=50, tol=1e-4,
                         return_info=False):
        """(N, 2) float64 points (x, y) through a registration (include/microaligner_flowinvert.h): "to_moving" takes
        points of the registered frame to the coordinate of the moving image that Warper samples there, "to_reference"
        takes points of the moving image to the registered frame by solving p - flow(p) = tmat . point.  tmat / image_shape:
        Warper.tmat and the shape of the moving image it resamples.  numpy points in and out; flow numpy or device
        resident, or a FlowGrid (sampled from its nodes in float64, include/microaligner_flowgrid.h).  With return_info a
        PointsInfo(converged, inside) of bool arrays beside the points."""
        pts, code, mat, left, top, max_iter, tol = transform_points_params(points, flow, direction, tmat, image_shape,
                                                                           max_iter, tol)
        grid = flow if isinstance(flow, FlowGrid) else None
        flow = self._grid_nodes(grid) if grid is not None else self.asdevice(flow)
        n = pts.shape[0]
        H, W = grid.shape if grid is not None else flow.shape[:2]
        d_pts, d_conv, d_in = self._upload_raw(pts), self._raw(n), self._raw(n)
        mat = None if mat is None else (C.c_double * 6)(*[float(v) for v in mat])
        m6, t6 = (mat, None) if code == L.MA_POINTS_TO_MOVING else (None, mat)
        if grid is not None:
            self._run(self.lib.ma_transform_points_grid, d_pts.ptr, n, flow.ptr, H, W, grid.stride, m6, t6, left, top, code,
                      max_iter, tol, d_pts.ptr, d_conv.ptr, d_in.ptr)
        else:
            self._run(self.lib.ma_transform_points, d_pts.ptr, n, flow.ptr, H, W, m6, t6, left, top, code, max_iter, tol,
                      d_pts.ptr, d_conv.ptr, d_in.ptr)
        out = self.download_raw(d_pts, (n, 2), np.float64)
        if not return_info:
            return out
        return out, PointsInfo(self.download_raw(d_conv, (n,), np.uint8).astype(bool),
                               self.download_raw(d_in, (n,), np.uint8).astype(bool))

    # thin-plate spline of landmark pairs (include/microaligner_landmarks.h) -------------------------------------------------
    def landmark_flow(self, cw, a6, c, k, shape, stride=1):
        """The flow of the spline (records cw, affine part a6, centre c, scale k: a LandmarkFit's) on the nodes of the grid of
        an (H, W) flow at `stride`: a DeviceArray (g(H, stride), g(W, stride), 2) float32; stride 1 is the dense flow."""
        cw, a6, cx, cy, k, H, W, stride = landmark_flow_params(cw, a6, c, k, shape, stride)
        d_cw = self._upload_raw(cw)
        out = self.empty((grid_nodes(H, stride), grid_nodes(W, stride), 2), np.float32)
        self._run(self.lib.ma_landmark_flow, d_cw.ptr, cw.shape[0], (C.c_double * 6)(*a6), cx, cy, k, H, W, stride, out.ptr)
        return out

    def landmark_points(self, cw, a6, c, k, points):
        """The spline's sampling map s at (N, 2) float64 points (x, y): numpy in, a new (N, 2) float64 array out."""
        cw, a6, cx, cy, k, pts = landmark_points_params(cw, a6, c, k, points)
        d_cw, d_pts = self._upload_raw(cw), self._upload_raw(pts)
        self._run(self.lib.ma_landmark_points, d_cw.ptr, cw.shape[0], (C.c_double * 6)(*a6), cx, cy, k, d_pts.ptr,
                  pts.shape[0], d_pts.ptr)
        return self.download_raw(d_pts, (pts.shape[0], 2), np.float64)

    def pyr_down(self, img, minmax=False):
        h, w = img.shape
        out = self.empty(((h + 1) // 2, (w + 1) // 2), img.dtype)
        if minmax:
            out.minmax = self.empty((2,), np.float32)
            self._run(self.lib.ma_pyr_down_minmax, img.ptr, _dt(img.dtype), h, w, out.ptr, out.minmax.ptr)
        else:
            self._run(self.lib.ma_pyr_down, img.ptr, _dt(img.dtype), h, w, out.ptr)
        return out

    def pyr_up_flow(self, flow, dst_hw, scale=1.0):
        """cv2.pyrUp(flow * scale, dstsize=(W, H)) with dst_hw = (H, W)."""
        h, w = flow.shape[:2]
        dh, dw = dst_hw
        out = self.empty((dh, dw, 2), np.float32)
        self._run(self.lib.ma_pyr_up_flow, flow.ptr, h, w, float(scale), out.ptr, int(dh), int(dw))
        return out

    def minmax(self, arr):
        mn, mx = C.c_double(), C.c_double()
        self._run(self.lib.ma_minmax, arr.ptr, _dt(arr.dtype), arr.size, C.byref(mn), C.byref(mx))
        return mn.value, mx.value

    def dog_u8(self, img, low_sigma=5, high_sigma=9, report_zero=False, flags=0):
        """Body of OptFlowRegistrator.dog -> uint8.  Stream ordered (no host sync) unless report_zero, in which
        case (out, src_max_is_zero) is returned; out is all zero when the input's max is 0.
        flags: rounding model of the chain (MA_DOG_FUSED_BLUR | MA_DOG_FUSED_SCALE, include/microaligner_hip.h)."""
        h, w = img.shape
        out = self.empty((h, w), np.uint8)
        if report_zero == "deferred":
            # no host sync: the flag lands in a page-locked word in stream order; any_deferred_zero() reads the words
            # handed out since its last call once the stream has been waited for (FeatureRegistrator's fast path)
            slot = self._zero_flag_slot()
            self._run(self.lib.ma_dog_u8_ex, img.ptr, _dt(img.dtype), h, w, int(low_sigma), int(high_sigma),
                      int(flags) | L.MA_DOG_REPORT_ASYNC, img.minmax.ptr if img.minmax is not None else None, out.ptr,
                      C.cast(C.c_void_p(self._zero_flags_ptr + 4 * slot), C.POINTER(C.c_int)))
            return out
        flag = C.c_int(0)
        fl = C.byref(flag) if report_zero else None
        # img.minmax: the producing kernel already reduced the image
        self._run(self.lib.ma_dog_u8_ex, img.ptr, _dt(img.dtype), h, w, int(low_sigma), int(high_sigma), int(flags),
                  img.minmax.ptr if img.minmax is not None else None, out.ptr, fl)
        return (out, bool(flag.value)) if report_zero else out

    _ZERO_FLAG_SLOTS = 1024

    def _zero_flag_slot(self):
        if getattr(self, "_zero_flags_ptr", None) is None:
            p = C.c_void_p()
            L.check(self.lib.ma_host_alloc(4 * self._ZERO_FLAG_SLOTS, C.byref(p)))
            self._zero_flags_ptr = p.value
            self._zero_flags = np.frombuffer((C.c_int * self._ZERO_FLAG_SLOTS).from_address(p.value), np.int32)
            self._zero_pending, self._zero_next, self._zero_carry = [], 0, False
        if len(self._zero_pending) >= self._ZERO_FLAG_SLOTS and self._settle_zero_flags():
            self._zero_carry = True             # ring full: what was pending is settled (synchronises) and remembered
        slot = self._zero_next
        self._zero_next = (slot + 1) % self._ZERO_FLAG_SLOTS
        self._zero_flags[slot] = 0              # not pending: no copy into it is in flight
        self._zero_pending.append(slot)
        return slot

    def _settle_zero_flags(self):
        pending = getattr(self, "_zero_pending", None)
        if not pending:
            return False
        self.sync()
        hit = bool(self._zero_flags[pending].any())
        pending.clear()
        return hit

    def any_deferred_zero(self):
        """True if any dog_u8(report_zero="deferred") since the last call saw an input whose max() is 0.  Waits for the
        stream (a no-op when the caller has just synchronised, e.g. by downloading scores)."""
        hit = self._settle_zero_flags() or getattr(self, "_zero_carry", False)
        self._zero_carry = False
        return hit

    def nmi_scores(self, a, b, chunk=0):
        if a.dtype != np.uint8 or b.dtype != np.uint8 or a.size != b.size:
            raise ValueError("NMI inputs must be uint8 arrays of equal size")
        n = a.size
        nch = 1 if (chunk <= 0 or chunk >= n) else (n + chunk - 1) // chunk
        scores = (C.c_double * nch)()
        got = C.c_int()
        self._run(self.lib.ma_nmi_u8, a.ptr, b.ptr, n, int(max(chunk, 0)), scores, nch, C.byref(got))
        return np.frombuffer(scores, dtype=np.float64, count=got.value).copy()

    def nmi_scores_pair(self, a, b0, b1, chunk=0):
        """Both halves of the gate in one call (ma_nmi_u8_pair): (scores of NMI(a, b0), scores of NMI(a, b1))."""
        for b in (b0, b1):
            if a.dtype != np.uint8 or b.dtype != np.uint8 or a.size != b.size:
                raise ValueError("NMI inputs must be uint8 arrays of equal size")
        n = a.size
        nch = 1 if (chunk <= 0 or chunk >= n) else (n + chunk - 1) // chunk
        s0, s1 = (C.c_double * nch)(), (C.c_double * nch)()
        got = C.c_int()
        self._run(self.lib.ma_nmi_u8_pair, a.ptr, b0.ptr, b1.ptr, n, int(max(chunk, 0)), s0, s1, nch, C.byref(got))
        return (np.frombuffer(s0, dtype=np.float64, count=got.value).copy(),
                np.frombuffer(s1, dtype=np.float64, count=got.value).copy())

    # per-cell maps: the checks and the grid shape the three calls below share -----------------------------------------
    @staticmethod
    def _check_cell_labels(ref, b0, b1, what):
        for b in (b0, b1):
            if b is not None and (ref.dtype != np.uint8 or b.dtype != np.uint8 or ref.shape != b.shape or ref.ndim != 2):
                raise ValueError(f"{what} labels must be 2-D uint8 arrays of equal shape")

    @staticmethod
    def _cell_grid_shape(h, w, cell_h, cell_w):
        return -(-h // int(cell_h)), -(-w // int(cell_w))

    # registration quality maps (include/microaligner_qc.h) ------------------------------------------------------------
    def qc_nmi_grid(self, ref, b0, b1, cell_h, cell_w):
        """Per cell of the (cell_h, cell_w) grid: NMI and Pearson r of the u8 labels (ref, b0) and, unless b1 is None,
        (ref, b1).  -> (nmi0, nmi1, ncc0, ncc1), each (gy, gx) float64 (the b1 pair None without b1)."""
        self._check_cell_labels(ref, b0, b1, "QC")
        h, w = ref.shape
        gy, gx = self._cell_grid_shape(h, w, cell_h, cell_w)
        pd = C.POINTER(C.c_double)
        nmi0, ncc0 = np.empty((gy, gx)), np.empty((gy, gx))
        nmi1, ncc1 = (np.empty((gy, gx)), np.empty((gy, gx))) if b1 is not None else (None, None)
        self._run(self.lib.ma_qc_nmi_grid, ref.ptr, b0.ptr, b1.ptr if b1 is not None else None, h, w, int(cell_h), int(cell_w),
                  nmi0.ctypes.data_as(pd), nmi1.ctypes.data_as(pd) if nmi1 is not None else None, ncc0.ctypes.data_as(pd),
                  ncc1.ctypes.data_as(pd) if ncc1 is not None else None)
        return nmi0, nmi1, ncc0, ncc1

    def qc_flow_grid(self, flow, cell_h, cell_w):
        """Per cell of an (h, w, 2) float32 flow: (jac_min, folded, invalid, flow_mean, flow_max), each (gy, gx)."""
        if flow.dtype != np.float32 or flow.ndim != 3 or flow.shape[2] != 2:
            raise ValueError(f"flow must be float32 of shape (H, W, 2), got {flow.dtype} {flow.shape}")
        h, w = flow.shape[:2]
        gy, gx = self._cell_grid_shape(h, w, cell_h, cell_w)
        pd, pl = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
        jmin, mean, mx = np.empty((gy, gx)), np.empty((gy, gx)), np.empty((gy, gx))
        folded, invalid = np.empty((gy, gx), np.int64), np.empty((gy, gx), np.int64)
        self._run(self.lib.ma_qc_flow_grid, flow.ptr, h, w, int(cell_h), int(cell_w), jmin.ctypes.data_as(pd),
                  folded.ctypes.data_as(pl), invalid.ctypes.data_as(pl), mean.ctypes.data_as(pd), mx.ctypes.data_as(pd))
        return jmin, folded, invalid, mean, mx

    # residual shift maps (include/microaligner_residual.h) ------------------------------------------------------------
    def residual_shift_grid(self, ref, b0, b1, cell_h, cell_w, max_shift, table=False):
        """Per cell of the (cell_h, cell_w) grid: the ZNCC peak within +-max_shift px of the u8 labels (ref, b0) and, unless
        b1 is None, (ref, b1).  -> (maps0, maps1), each a dict of (gy, gx) arrays shift_x, shift_y, score, score0 (float64),
        at_limit, valid (bool) and table ((gy, gx, 2R + 1, 2R + 1) float64, or None without table=True); maps1 is None
        without b1."""
        self._check_cell_labels(ref, b0, b1, "residual shift")
        h, w = ref.shape
        R = int(max_shift)
        gy, gx = self._cell_grid_shape(h, w, cell_h, cell_w)
        pd, pb = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)

        def outputs(wanted):
            if not wanted:
                return None, [None] * 7
            m = {k: np.empty((gy, gx)) for k in ("shift_x", "shift_y", "score", "score0")}
            m["at_limit"], m["valid"] = np.empty((gy, gx), np.uint8), np.empty((gy, gx), np.uint8)
            m["table"] = np.empty((gy, gx, 2 * R + 1, 2 * R + 1)) if table else None
            return m, [m[k].ctypes.data_as(pd) for k in ("shift_x", "shift_y", "score", "score0")] + \
                [m[k].ctypes.data_as(pb) for k in ("at_limit", "valid")] + \
                [m["table"].ctypes.data_as(pd) if table else None]
        m0, p0 = outputs(True)
        m1, p1 = outputs(b1 is not None)
        self._run(self.lib.ma_residual_shift_grid, ref.ptr, b0.ptr, b1.ptr if b1 is not None else None, h, w, int(cell_h),
                  int(cell_w), R, *p0, *p1)
        for m in (m0, m1):
            if m is not None:
                m["at_limit"], m["valid"] = m["at_limit"].astype(bool), m["valid"].astype(bool)
        return m0, m1

    # global translation search (include/microaligner_translation.h) ----------------------------------------------------
    def translation_moments(self, ref, mov, window):
        """The five integer moments of the u8 labels (ref, mov) at every shift of window = (dx0, dx1, dy0, dy1), each over
        that shift's overlap -> (5, ny, nx) uint64 in the order S_ab, S_a, S_aa, S_b, S_bb, entry [dy - dy0, dx - dx0]."""
        h, w, dx0, dx1, dy0, dy1, _ = translation_params(ref, mov, window)
        mom = np.empty((5, dy1 - dy0 + 1, dx1 - dx0 + 1), np.uint64)
        self._run(self.lib.ma_translation_moments, ref.ptr, mov.ptr, h, w, dx0, dx1, dy0, dy1,
                  mom.ctypes.data_as(C.POINTER(C.c_ulonglong)))
        return mom

    def translation_search(self, ref, mov, window, exclude=2, table=False):
        """The ZNCC peak of the u8 labels (ref, mov) over window = (dx0, dx1, dy0, dy1) -> a dict of dx, dy (int), delta_x,
        delta_y, score, second (float), n (int), at_limit, valid (bool) and table ((ny, nx) float64 of all scores, or None
        without table=True)."""
        h, w, dx0, dx1, dy0, dy1, exclude = translation_params(ref, mov, window, exclude)
        res = L.TranslationResult()
        tab = np.empty((dy1 - dy0 + 1, dx1 - dx0 + 1)) if table else None
        self._run(self.lib.ma_translation_search, ref.ptr, mov.ptr, h, w, dx0, dx1, dy0, dy1, exclude, C.byref(res),
                  tab.ctypes.data_as(C.POINTER(C.c_double)) if table else None)
        return dict(dx=int(res.dx), dy=int(res.dy), delta_x=float(res.delta_x), delta_y=float(res.delta_y),
                    score=float(res.score), second=float(res.second), n=int(res.n), at_limit=bool(res.at_limit),
                    valid=bool(res.valid), table=tab)

    def max_project(self, stack):
        nz = stack.shape[0]
        out = self.empty(stack.shape[1:], stack.dtype)
        self._run(self.lib.ma_max_project, stack.ptr, _dt(stack.dtype), nz, out.size, out.ptr)
        return out

    def warp_affine(self, img, inverse_3x3):
        """skimage.transform.warp(img, AffineTransform(inverse_3x3), preserve_range=True).astype(img.dtype)."""
        h, w = img.shape
        m = (C.c_double * 9)(*[float(v) for v in np.asarray(inverse_3x3, dtype=np.float64).ravel()])
        out = self.empty((h, w), img.dtype)
        self._run(self.lib.ma_warp_affine, img.ptr, _dt(img.dtype), h, w, m, out.ptr)
        return out

    def warp_affine_cv(self, img, m2x3, dsize=None):
        """cv2.warpAffine(img, m2x3, dsize=(W, H)) with the default flags (bilinear, constant border 0)."""
        h, w = img.shape
        dw, dh = (w, h) if dsize is None else (int(dsize[0]), int(dsize[1]))
        m = np.asarray(m2x3, dtype=np.float64)
        if m.shape != (2, 3):
            raise ValueError("the transform must be a 2x3 matrix")
        mm = (C.c_double * 6)(*[float(v) for v in m.ravel()])
        out = self.empty((dh, dw), img.dtype)
        self._run(self.lib.ma_warp_affine_cv, img.ptr, _dt(img.dtype), h, w, mm, dh, dw, out.ptr)
        return out

    def knn2(self, query, train, mode="auto", stats=None, on_device=False):
        """Exact 2-NN (L2) of every row of `query` among the rows of `train`: (idx (n, 2) int64, dist (n, 2) float32)
        on the host, like feature_reg.sparse_cpu.knn2.  Either side may be a host array or a DeviceArray (descriptors
        that ma_daisy_describe left on the device are searched where they are).
        mode: "auto" | "exact" | "filtered" | "filtered_f32" (ma_knn2_l2_ex: matrix-core shortlist -- split-float16 or FP32 --
        + exact re-evaluation + certificate; the same result bit for bit); stats: a dict that receives {"uncertified": queries served by the exact fallback}.
        on_device: leave the results where they are -- (idx (n, 2) int32 bits, SQUARED dist (n, 2) float32) device buffers, what
        match_similarity takes."""
        modes = {"auto": L.MA_KNN_AUTO, "exact": L.MA_KNN_EXACT, "filtered": L.MA_KNN_FILTERED, "filtered_f32": L.MA_KNN_FILTERED_F32}
        if mode not in modes:
            raise ValueError(f"unknown search mode {mode!r}: auto, exact, filtered or filtered_f32")
        def prep(a):
            if isinstance(a, DeviceArray):
                if a.ndim != 2 or a.dtype != np.float32 or a.shape[1] % 4:
                    raise ValueError("device descriptors must be (n, dim) float32 with dim a multiple of 4")
                return a
            a = np.ascontiguousarray(a, np.float32)
            if a.ndim != 2:
                raise ValueError("query and train must be 2-D")
            pad = -a.shape[1] % 4
            return self.asdevice(np.pad(a, ((0, 0), (0, pad))) if pad else a)
        dq, dt = prep(query), prep(train)
        if dq.shape[1] != dt.shape[1]:
            raise ValueError("query and train must have the same descriptor length")
        nq = dq.shape[0]
        # (the image dtypes of asdevice() do not include int32: raw buffers for the results)
        idx, dist = self.empty((nq, 2), np.float32), self.empty((nq, 2), np.float32)
        unc = C.c_int(0)
        self._run(self.lib.ma_knn2_l2_ex, dq.ptr, nq, dt.ptr, dt.shape[0], dq.shape[1], idx.ptr, dist.ptr, modes[mode],
                  C.byref(unc) if stats is not None else None)
        if stats is not None:
            stats["uncertified"] = unc.value
        if on_device:
            return idx, dist
        out_i = np.empty((nq, 2), np.int32)
        L.check(self.lib.ma_memcpy_d2h(self.handle, out_i.ctypes.data, idx.ptr, out_i.nbytes))
        return out_i.astype(np.int64), np.sqrt(dist.numpy())   # the kernel returns squared distances

    _PCG64_STATES = {}

    def match_similarity(self, idx, dist_sq, query_pts, train_pts, ratio=0.5, confidence=0.99, reproj_threshold=3.0,
                         max_iters=2000, seed=0, n_train=None):
        """Ratio test + RANSAC similarity fit on the device (ma_match_similarity) over what knn2(on_device=True) left there:
        bit for bit feature_reg.sparse_cpu.estimate_affine_partial_2d(query points of the good matches, their train points).
        query_pts / train_pts: (n, 2) float64 device buffers (x, y).  n_train: the number of train points -- a match whose first
        neighbour is not in [0, n_train) is not a good match; None: what train_pts holds, nbytes // 16 (a buffer of capacity
        size then guards nothing: pass the count).  Returns (matrix (2, 3) float64 or None, n_good, status);
        status as in include/microaligner_hip.h: 0 ok, 1 fewer than 3 good matches, 2 no model, 3 not computed (use the host)."""
        st = self._PCG64_STATES.get(seed)
        if st is None:     # numpy's seeding (SeedSequence -> PCG64) stays numpy's: only the stream is restated in C
            raw = np.random.PCG64(seed).state["state"]
            m64 = (1 << 64) - 1
            st = self._PCG64_STATES[seed] = (C.c_ulonglong * 4)(raw["state"] >> 64, raw["state"] & m64, raw["inc"] >> 64,
                                                                raw["inc"] & m64)
        nq = int(idx.nbytes // 8)             # (nq, 2) int32, typed (knn2) or raw (tests)
        mat = (C.c_double * 6)()
        n_good, status = C.c_int(0), C.c_int(0)
        nt = int(train_pts.nbytes // 16)
        if n_train is not None:
            if not 0 <= int(n_train) <= nt:
                raise ValueError(f"n_train = {n_train} does not fit the train points buffer ({nt} points)")
            nt = int(n_train)
        self._run(self.lib.ma_match_similarity, idx.ptr, dist_sq.ptr, nq, query_pts.ptr, train_pts.ptr,
                  nt, float(ratio), float(confidence), float(reproj_threshold), int(max_iters), st, mat,
                  C.byref(n_good), C.byref(status))
        m = np.array(mat, np.float64).reshape(2, 3) if status.value == 0 else None
        return m, n_good.value, status.value

    def cut_tiles(self, img, tile, overlap, first_tile, n_tiles):
        """The zero-padded feature windows first_tile .. first_tile + n_tiles of a uint8 device image: (n, P, P)."""
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("FAST works on uint8 images (the DOG output)")
        H, W = img.shape
        P = tile + 2 * overlap
        out = self.empty((n_tiles, P, P), np.uint8)
        self._run(self.lib.ma_cut_tiles_u8, img.ptr, H, W, int(tile), int(overlap), int(first_tile), int(n_tiles), out.ptr)
        return out

    def fast_keypoints(self, tiles, margin, limit, threshold=1):
        """FAST-9/16 corners of every tile interior, strongest `limit` first (row-major among equals), selected on the
        device: (counts (nt,), kp (nt, limit, 3) int32 = x, y, response; rows beyond counts[t] are undefined)."""
        nt, P, P2 = tiles.shape
        if P != P2 or tiles.dtype != np.uint8:
            raise ValueError("FAST works on square uint8 tiles (the DOG output)")
        out = self._raw(nt * limit * 3 * 4)
        counts = (C.c_int * nt)()
        self._run(self.lib.ma_fast_keypoints, tiles.ptr, nt, P, int(margin), int(threshold), int(limit), out.ptr, counts)
        host = np.empty((nt, limit, 3), np.int32)
        L.check(self.lib.ma_memcpy_d2h(self.handle, host.ctypes.data, out.ptr, host.nbytes))
        return np.frombuffer(counts, np.int32).copy(), host

    def _raw(self, nbytes):
        """Untyped HBM buffer from the pool (results that are not image dtypes: int32 scores, float64 points)."""
        return self.empty((max(int(nbytes), 1),), np.uint8)

    def _upload_raw(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = self._raw(arr.nbytes)
        if arr.nbytes:
            L.check(self.lib.ma_memcpy_h2d(self.handle, buf.ptr, arr.ctypes.data, arr.nbytes))
        return buf

    def fast_nms(self, tiles, margin, threshold=1):
        """FAST-9/16 score at the 3x3 local maxima of every tile interior: (nt, P-2m, P-2m) int32 on the host."""
        nt, P, P2 = tiles.shape
        if P != P2 or tiles.dtype != np.uint8:
            raise ValueError("FAST works on square uint8 tiles (the DOG output)")
        Pi = P - 2 * margin
        out = self._raw(nt * Pi * Pi * 4)
        self._run(self.lib.ma_fast_nms, tiles.ptr, nt, P, int(margin), int(threshold), out.ptr)
        host = np.empty((nt, Pi, Pi), np.int32)
        L.check(self.lib.ma_memcpy_d2h(self.handle, host.ctypes.data, out.ptr, host.nbytes))
        return host

    def daisy_describe(self, tiles, kp_tile, kp_xy, weights, cos_sin, offsets, on_device=False):
        """DAISY descriptors at the given keypoints: (n, 200) float32 on the host, or left on the device (see
        ma_daisy_describe)."""
        nt, P, _ = tiles.shape
        n = len(kp_tile)
        d_tile = self._upload_raw(np.asarray(kp_tile, np.int32))
        d_xy = self._upload_raw(np.asarray(kp_xy, np.float64))
        desc = self.empty((n, 200), np.float32)
        halves = [np.ascontiguousarray(w, np.float64) for w in weights]
        wptr = (C.POINTER(C.c_double) * 3)(*[h.ctypes.data_as(C.POINTER(C.c_double)) for h in halves])
        radii = (C.c_int * 3)(*[len(h) - 1 for h in halves])
        cs = np.ascontiguousarray(cos_sin, np.float64)
        of = np.ascontiguousarray(offsets, np.float64)
        self._run(self.lib.ma_daisy_describe, tiles.ptr, _dt(tiles.dtype), nt, P, wptr, radii,
                  cs.ctypes.data_as(C.POINTER(C.c_double)), of.ctypes.data_as(C.POINTER(C.c_double)), d_tile.ptr, d_xy.ptr,
                  n, desc.ptr)
        return desc if on_device else desc.numpy()

    _COUNT_SLOTS = 256

    def _count_slot(self):
        """A page-locked int32 for a count that arrives in stream order (ma_feature_extract_enqueue): a view of one word of a
        small ring (a slot is read once, right after the event behind its call; 256 calls later it is handed out again)."""
        if getattr(self, "_count_ptr", None) is None:
            p = C.c_void_p()
            L.check(self.lib.ma_host_alloc(4 * self._COUNT_SLOTS, C.byref(p)))
            self._count_ptr = p.value
            self._count_words = np.frombuffer((C.c_int * self._COUNT_SLOTS).from_address(p.value), np.int32)
            self._count_next = 0
        k = self._count_next
        self._count_next = (k + 1) % self._COUNT_SLOTS
        self._count_words[k] = 0
        return self._count_words[k:k + 1], C.cast(C.c_void_p(self._count_ptr + 4 * k), C.POINTER(C.c_int))

    def feature_extract(self, img, tile, overlap, limit, weights, cos_sin, offsets, threshold=1, workspace_bytes=0, wait=True):
        """tile_registration.find_features of a uint8 device image in one call (ma_feature_extract): returns
        (descriptors (n, 200) float32 DeviceArray, points (n, 2) float64 raw device buffer, responses (n,) int32 raw device
        buffer, n); everything stays on the device, the keypoint count is the only thing that comes back.
        wait=False (ma_feature_extract_enqueue): nothing is waited for; n is a one-element int32 array on page-locked memory
        that holds the count once the stream has passed the call (the caller waits for an event recorded behind it), and
        the descriptor array keeps its capacity as its first dimension until then."""
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("FAST works on uint8 images (the DOG output)")
        H, W = img.shape
        n_tiles = -(-H // tile) * -(-W // tile)
        cap = n_tiles * int(limit)
        desc = self.empty((cap, 200), np.float32)
        pts, resp = self._raw(cap * 16), self._raw(cap * 4)
        halves = [np.ascontiguousarray(w, np.float64) for w in weights]
        wptr = (C.POINTER(C.c_double) * 3)(*[h.ctypes.data_as(C.POINTER(C.c_double)) for h in halves])
        radii = (C.c_int * 3)(*[len(h) - 1 for h in halves])
        cs = np.ascontiguousarray(cos_sin, np.float64)
        of = np.ascontiguousarray(offsets, np.float64)
        if not wait:
            word, wp = self._count_slot()
            self._run(self.lib.ma_feature_extract_enqueue, img.ptr, H, W, int(tile), int(overlap), int(threshold), int(limit), wptr,
                      radii, cs.ctypes.data_as(C.POINTER(C.c_double)), of.ctypes.data_as(C.POINTER(C.c_double)),
                      int(workspace_bytes), cap, desc.ptr, pts.ptr, resp.ptr, wp)
            return desc, pts, resp, word
        n = C.c_int(0)
        self._run(self.lib.ma_feature_extract, img.ptr, H, W, int(tile), int(overlap), int(threshold), int(limit), wptr, radii,
                  cs.ctypes.data_as(C.POINTER(C.c_double)), of.ctypes.data_as(C.POINTER(C.c_double)), int(workspace_bytes), cap,
                  desc.ptr, pts.ptr, resp.ptr, C.byref(n))
        desc.shape = (n.value, 200)
        return desc, pts, resp, n.value

    def feature_round(self, current, current_gate, ref_gate, ref_features, tile, use_dog, nmi_chunk, weights, cos_sin, offsets,
                      workspace_bytes=0):
        """One round of FeatureRegistrator's level loop in one call (ma_feature_round).  current: the level's moving image
        (DeviceArray); current_gate: dog(current) or None (then it is computed and returned); ref_gate: dog(reference level);
        ref_features: (descriptors DeviceArray (n, 200), points raw buffer, n) of the reference level or None.  Returns a dict:
        estimate (2, 3), n_query, n_good, status, is_identity, zero_max, scores_after, scores_before (per chunk), current_gate,
        candidate, candidate_gate (the last two None for an identity estimate)."""
        H, W = current.shape
        made_gate = current_gate is None
        gate_out = self.empty((H, W), np.uint8) if made_gate else None
        cand, cand_gate = self.empty((H, W), current.dtype), self.empty((H, W), np.uint8)
        n = H * W
        nch = 1 if (nmi_chunk <= 0 or nmi_chunk >= n) else (n + nmi_chunk - 1) // nmi_chunk
        s_after, s_before = (C.c_double * nch)(), (C.c_double * nch)()
        halves = [np.ascontiguousarray(w, np.float64) for w in weights]
        wptr = (C.POINTER(C.c_double) * 3)(*[h.ctypes.data_as(C.POINTER(C.c_double)) for h in halves])
        radii = (C.c_int * 3)(*[len(h) - 1 for h in halves])
        cs = np.ascontiguousarray(cos_sin, np.float64)
        of = np.ascontiguousarray(offsets, np.float64)
        res = L.MaFeatureRoundResult()
        rdesc, rpts, rn = ref_features if ref_features is not None else (None, None, 0)
        self._run(self.lib.ma_feature_round, current.ptr, _dt(current.dtype), H, W,
                  None if made_gate else current_gate.ptr, gate_out.ptr if made_gate else None, ref_gate.ptr,
                  rdesc.ptr if rn else None, rpts.ptr if rn else None, int(rn), int(tile), 1 if use_dog else 0,
                  int(max(nmi_chunk, 0)), wptr, radii, cs.ctypes.data_as(C.POINTER(C.c_double)),
                  of.ctypes.data_as(C.POINTER(C.c_double)), int(workspace_bytes), cand.ptr, cand_gate.ptr, s_after, s_before, nch,
                  C.byref(res))
        ident = bool(res.is_identity)
        return dict(estimate=np.array(list(res.m2x3), np.float64).reshape(2, 3), n_query=res.n_query, n_good=res.n_good,
                    status=res.status, is_identity=ident, zero_max=res.zero_max,
                    scores_after=np.frombuffer(s_after, np.float64, res.n_scores).copy(),
                    scores_before=np.frombuffer(s_before, np.float64, res.n_scores).copy(),
                    current_gate=gate_out if made_gate else current_gate,
                    candidate=None if ident else cand, candidate_gate=None if ident else cand_gate)

    def download_raw(self, buf, shape, dtype):
        """A raw device buffer (_raw) as a host array of the given shape and dtype."""
        out = np.empty(shape, dtype)
        if out.nbytes:
            L.check(self.lib.ma_memcpy_d2h(self.handle, out.ctypes.data, buf.ptr, out.nbytes))
        return out

    def to_f32(self, arr):
        """Mat::convertTo(CV_32F): exact for the integer dtypes (ma_convert_f32); float32 arrays pass through."""
        if arr.dtype == np.float32:
            return arr
        out = self.empty(arr.shape, np.float32)
        self._run(self.lib.ma_convert_f32, arr.ptr, _dt(arr.dtype), arr.size, out.ptr)
        return out

    def normalize_minmax_u8(self, arr):
        out = self.empty(arr.shape, np.uint8)
        self._run(self.lib.ma_normalize_minmax_u8, arr.ptr, _dt(arr.dtype), arr.size, out.ptr)
        return out

    # order statistics and range normalisation (include/microaligner_quantile.h) ----------------------------------------
    def image_quantiles(self, arr, q, ignore_zeros=False):
        """The order statistics q (each in [0, 1], at most 8, numpy's method="lower") of a uint8 / uint16 / float32 device
        array over its finite pixels -- without its zeros with ignore_zeros -> (values as a float64 array, NaN for an empty
        population; QuantileCounts(pop, nonfinite, zeros))."""
        dt, n, qs, flags = image_quantiles_params(arr, q, ignore_zeros)
        values = np.empty(qs.size, np.float64)
        counts = (C.c_longlong * 3)()
        self._run(self.lib.ma_image_quantiles, arr.ptr, dt, n, flags, qs.ctypes.data_as(C.POINTER(C.c_double)), int(qs.size),
                  values.ctypes.data_as(C.POINTER(C.c_double)), counts)
        return values, QuantileCounts(int(counts[0]), int(counts[1]), int(counts[2]))

    def normalize_range_u8(self, arr, lo, hi):
        """arr scaled so that lo -> 0 and hi -> 255, clamped and rounded half to even -> a uint8 DeviceArray; all zeros for
        hi <= lo.  Stream ordered."""
        dt, n, lo, hi = normalize_range_params(arr, lo, hi)
        out = self.empty(arr.shape, np.uint8)
        self._run(self.lib.ma_normalize_range_u8, arr.ptr, dt, n, lo, hi, out.ptr)
        return out


_contexts = {}
_contexts_lock = threading.Lock()
_tls = threading.local()


class use_context:
    """`with use_context(ctx):` makes `ctx` the context get_context() returns on this thread.  Several contexts
    (each with its own HIP stream, workspace and buffer pool) can drive one device from different threads: that is
    how independent (ref, mov) pairs are kept in flight together (parallel.register_pairs(lanes=...))."""

    def __init__(self, ctx):
        self.ctx, self.prev = ctx, None

    def __enter__(self):
        self.prev = getattr(_tls, "ctx", None)
        _tls.ctx = self.ctx
        return self.ctx

    def __exit__(self, *exc):
        _tls.ctx = self.prev
        return False


def default_device():
    """Device index for this process: MICROALIGNER_DEVICE, else LOCAL_RANK (one process per GPU), else 0."""
    for var in ("MICROALIGNER_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v is not None and v != "":
            return int(v)
    return 0


def get_context(device=None):
    """Process-wide context of a device (created on first use).  Raises when no HIP device exists."""
    if device is None:
        cur = getattr(_tls, "ctx", None)
        if cur is not None:
            return cur
        device = default_device()
    with _contexts_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            n = C.c_int()
            lib = L.load()
            lib.ma_device_count(C.byref(n))
            if n.value > 0 and not 0 <= device < n.value:
                # no silent wrap-around: a LOCAL_RANK beyond the visible devices would double-book a GPU
                raise ValueError(f"HIP device index {device} is out of range: {n.value} device(s) visible "
                                 "(MICROALIGNER_DEVICE / LOCAL_RANK select the device of this process)")
            ctx = _contexts[device] = Context(device)
    return ctx


def _parse_cpulist(text):
    """"0-63,128-191" -> sorted list of CPU indices (the format of sysfs cpulist files)."""
    cpus = set()
    for part in text.strip().split(","):
        part = part.strip()
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return sorted(cpus)


def device_local_cpus(device=0, pci_bus_id=None, sysfs="/sys/bus/pci/devices"):
    """CPUs of the NUMA node a device hangs off (/sys/bus/pci/devices/<bdf>/local_cpulist), [] when unknown."""
    try:
        bdf = (pci_bus_id or device_info(device)["pci_bus_id"]).lower()
        with open(os.path.join(sysfs, bdf, "local_cpulist")) as f:
            return _parse_cpulist(f.read())
    except (OSError, ValueError, RuntimeError, KeyError):
        return []


def bind_to_device_numa(device=None, pci_bus_id=None, sysfs="/sys/bus/pci/devices"):
    """Pin this process (and every thread it starts afterwards) to the CPUs next to its GPU, so that the page-locked
    transfer buffers it allocates from now on and the pages its loaders first touch are on the memory the GPU reaches
    without crossing the socket interconnect: on a two-socket host a remote buffer costs a third of the PCIe rate
    (profiles/r04_notes.md).  One process per GPU: call it first thing in a rank.  Returns the CPU list it
    applied ([] when the topology is unknown or MICROALIGNER_BIND_NUMA=0: nothing changed); the previous mask is returned
    by os.sched_getaffinity before the call if the caller wants to restore it."""
    if os.environ.get("MICROALIGNER_BIND_NUMA", "1") == "0":
        return []
    cpus = device_local_cpus(default_device() if device is None else device, pci_bus_id, sysfs)
    allowed = os.sched_getaffinity(0)
    cpus = [c for c in cpus if c in allowed]
    if not cpus or set(cpus) == set(allowed):
        return []
    set_affinity(cpus)
    return cpus


def set_affinity(cpus):
    """Affinity of EVERY thread of this process (sched_setaffinity(0, ...) alone moves the calling thread only; the HIP
    runtime's helper threads, which carry the staged copies, exist already once a device has been queried)."""
    try:
        tids = [int(t) for t in os.listdir("/proc/self/task")]
    except OSError:
        tids = [0]
    for tid in tids:
        try:
            # the library's staging-copy workers are pinned one per L3 domain (ma_api.hip CopyPool): they keep their
            # placement, restricted to the new set where the two intersect
            with open(f"/proc/self/task/{tid}/comm") as f:
                if f.read().startswith("ma-copy-"):
                    keep = os.sched_getaffinity(tid) & set(cpus)
                    if keep:
                        os.sched_setaffinity(tid, keep)
                        continue
        except OSError:
            pass
        try:
            os.sched_setaffinity(tid, cpus)
        except OSError:
            pass        # a thread that exited in the meantime
    os.sched_setaffinity(0, cpus)


def host_register(arr):
    """Page-lock `arr`'s memory in place (ma_host_register): transfers to and from it then go by DMA directly instead of
    through the staging chunks -- one pass over host DRAM per byte instead of three.  For arrays that live across many
    transfers (parallel.shared_array results, reused input buffers); registration itself costs about a first touch of
    every page.  Returns True when the range is page-locked now, False when nothing was registered: the runtime refused
    (no device in this process, pages that cannot be pinned -- a memmap of a file on disk), or `arr` is not an ndarray /
    memmap whose memory outlives the call (a list would be converted to a temporary, and a registration must never outlive
    its memory), or no finalizer can be attached to the object that owns the memory.  The array then goes through the
    staging path as before.  The registration ends with the array (weakref finalizer on its owner)."""
    import weakref
    if not isinstance(arr, np.ndarray) or arr.nbytes == 0 or not arr.flags.c_contiguous:
        return False
    base = arr
    while isinstance(getattr(base, "base", None), np.ndarray):     # the finalizer hangs on the object that owns the memory
        base = base.base
    lib = L.load()
    ptr = arr.ctypes.data
    if lib.ma_host_register(C.c_void_p(ptr), C.c_size_t(arr.nbytes)) != L.MA_OK:
        return False
    try:
        # (the finalizer must run BEFORE the memory is unmapped: it hangs on the owning ndarray / memmap, whose death precedes
        # the release of its buffer)
        weakref.finalize(base, lib.ma_host_unregister, C.c_void_p(ptr))
    except TypeError:          # not weak-referenceable: nothing would ever end the registration
        lib.ma_host_unregister(C.c_void_p(ptr))
        return False
    return True


def host_unregister(arr):
    """End a registration made by host_register(arr) now (its finalizer later finds nothing left to do)."""
    if isinstance(arr, np.ndarray) and arr.nbytes:
        return L.load().ma_host_unregister(C.c_void_p(arr.ctypes.data)) == L.MA_OK
    return False


def transfer_mode(arr):
    """How a blocking transfer to / from the whole of `arr` is carried out (ma_host_transfer_is_direct): "direct" -- page-locked
    over its full extent, DMA as it is; "transient" -- pageable, but the copy page-locks the range for its own duration (opt-in:
    MICROALIGNER_TRANSIENT_PIN=1, arrays of >= 64 MiB); "staged" -- through the page-locked ring."""
    a = np.asarray(arr)
    if a.nbytes == 0:
        return "staged"
    out = C.c_int(0)
    L.check(L.load().ma_host_transfer_is_direct(C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.byref(out)))
    return {1: "direct", 2: "transient"}.get(out.value, "staged")


def transient_pin_stats():
    """dict(copies, slow_registrations, register_ms, gib, active) of the transient page-locking in this process
    (ma_transient_pin_stats)."""
    c, sl, ms, gib, act = C.c_longlong(), C.c_longlong(), C.c_double(), C.c_double(), C.c_int()
    L.check(L.load().ma_transient_pin_stats(C.byref(c), C.byref(sl), C.byref(ms), C.byref(gib), C.byref(act)))
    return dict(copies=c.value, slow_registrations=sl.value, register_ms=ms.value, gib=gib.value, active=bool(act.value))


def transfer_is_direct(arr):
    """Whether a transfer to / from the whole of `arr` goes by DMA as it is (page-locked over its full extent)."""
    return transfer_mode(arr) == "direct"


_STAGED_WARNED = [False]


def _warn_if_staged_on_a_full_node(arr):
    """beyond about three ranks per node the staged path (three to four passes over host DRAM per
    payload byte) cannot be the data plane.  Said once per process when a big pageable array reaches a transfer engine."""
    if _STAGED_WARNED[0] or arr.nbytes < (64 << 20):
        return
    try:
        ws = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    except ValueError:
        return
    if ws >= 3 and transfer_mode(arr) == "staged":
        import warnings
        _STAGED_WARNED[0] = True
        warnings.warn(f"microaligner_amd: a pageable {arr.nbytes >> 20} MiB array is going through the staged copy path with "
                      f"{ws} ranks on this node; the host's memory bandwidth will not carry that for every rank -- page-lock "
                      "buffers that are reused (device.host_register, parallel.shared_array, Context.host_empty)",
                      RuntimeWarning, stacklevel=3)


def device_count():
    n = C.c_int()
    L.load().ma_device_count(C.byref(n))
    return n.value


def device_info(device=0):
    """dict(name, pci_bus_id, mem_free, mem_total, compute_units) of a device (ma_device_info)."""
    name, pci = C.create_string_buffer(256), C.create_string_buffer(64)
    free, total, cus = C.c_size_t(), C.c_size_t(), C.c_int()
    L.check(L.load().ma_device_info(int(device), name, 256, pci, 64, C.byref(free), C.byref(total), C.byref(cus)))
    return dict(name=name.value.decode(), pci_bus_id=pci.value.decode(), mem_free=free.value, mem_total=total.value,
                compute_units=cus.value)
