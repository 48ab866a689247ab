"""Taking a flow apart (include/microaligner_flowaffine.h): the global affine part of a dense flow by weighted least
squares, the flow relative to a matrix and back, and the affine part per cell of a grid.  No counterpart in the reference.

    tmat = fit_flow_affine(f)                     the 2 x 3 matrix (Warper.tmat's convention) that leaves the least flow
    tmat, rest = split_flow(f)                    Warper(tmat=tmat, flow=rest) samples where Warper(flow=f) does
    f = join_flow(tmat, rest)                     ... and back
    maps = local_affine(f, cell_size=1000)        rotation, scale, anisotropy and shift per cell

The sums come from one pass over the flow on the device (Context.flow_affine_moments); the solve is a few float64
operations on the host (solve_flow_affine).  Every argument is checked before any device work.  numpy in, numpy out;
DeviceArray in, DeviceArray out (matrices and maps are always numpy).  A FlowGrid is expanded on the device first
(device.dense_flow) and gives the kind of array its nodes are.
"""
import collections
from dataclasses import dataclass

import numpy as np

from ..device import DeviceArray, FlowGrid, dense_flow, flow_affine_apply_params, flow_affine_moments_params, get_context

MODELS = ("affine", "similarity", "rigid", "translation")


class FlowAffineInfo(collections.namedtuple("FlowAffineInfo", "counts rms model centred residual_rms")):
    """fit_flow_affine / split_flow(..., return_info=True): the (used, invalid, unweighted, trimmed) pixel counts of every
    round (the untrimmed fit first), the weighted RMS of the flow over the last round's used pixels in px, the model (None
    where split_flow was given its matrix), the matrix in the centred frame, and -- from split_flow only, else None -- the
    weighted RMS of the residual flow."""


def _like(flow):
    return flow.nodes if isinstance(flow, FlowGrid) else flow


def _described(flow):
    """what the checks read of a flow: the flow itself, or for a FlowGrid an array of its expansion's shape and dtype that
    holds no memory, so that every argument is checked before the grid is expanded on the device"""
    return np.broadcast_to(np.float32(0), tuple(flow.shape) + (2,)) if isinstance(flow, FlowGrid) else flow


def _check_model(model):
    if not isinstance(model, str) or model not in MODELS:
        raise ValueError(f"unknown model {model!r}: expected one of {list(MODELS)}")
    return model


def _cell_weight(weight, cell_size, shape):
    # per-cell maps arrive from FlowQC / RegistrationQC as float64, int64 or bool: a host map of any real dtype that is
    # not a per-pixel one is rounded to the float32 the kernel reads (a few numbers per cell)
    if cell_size is not None and isinstance(weight, np.ndarray) and weight.dtype != np.float32 and \
            weight.dtype.kind in "biuf" and weight.shape != tuple(shape[:2]):
        return weight.astype(np.float32)
    return weight


def _centre(shape):
    return np.array([(shape[1] - 1) / 2.0, (shape[0] - 1) / 2.0])


def _to_absolute(centred, shape):
    """the centred-frame matrix (..., 2, 3) in absolute pixel coordinates: t_abs = c + t - L c"""
    c = _centre(shape)
    out = np.array(centred, dtype=np.float64)
    out[..., 2] = c + centred[..., 2] - centred[..., :2] @ c
    return out


def _to_centred(tmat, shape):
    c = _centre(shape)
    out = np.array(tmat, dtype=np.float64)
    out[..., 2] = tmat[..., 2] + tmat[..., :2] @ c - c
    return out


def solve_flow_affine(sums, model="affine"):
    """The fit from the 14 sums of include/microaligner_flowaffine.h, float64 on the host.  sums: (..., 14).
    -> (centred (..., 2, 3), deficient (...) bool): the matrix in the centred frame (it maps (a, b) to (X, Y)), NaN where
    the cell is deficient.

    With the weighted means subtracted, C the (unnormalised) covariance of s = (a, b) and K the cross-covariance of s with
    p = (X, Y): "affine" solves C L^T = K; "similarity" takes L = [[a, -b], [b, a]] with (a, b) = (tr, skew) / tr C,
    tr = K_aX + K_bY, skew = K_aY - K_bX; "rigid" takes the angle atan2(skew, tr); "translation" takes L = I.  The
    translation is mean(p) - L mean(s).  Deficient: sum w == 0; det C <= 1e-12 (tr C)^2 for "affine"; tr C <= 0 for
    "similarity" and "rigid"."""
    _check_model(model)
    S = np.asarray(sums, dtype=np.float64)
    if S.shape[-1] != 14:
        raise ValueError(f"sums must have 14 entries along the last axis, got {S.shape}")
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sw, sa, sb, saa, sab, sbb, sx, sy, sax, sbx, say, sby = (S[..., k] for k in range(12))
        ok = sw > 0
        swd = np.where(ok, sw, 1.0)
        ma, mb, mx, my = sa / swd, sb / swd, sx / swd, sy / swd
        caa, cab, cbb = saa - sa * ma, sab - sa * mb, sbb - sb * mb
        kax, kbx, kay, kby = sax - sa * mx, sbx - sb * mx, say - sa * my, sby - sb * my
        trc = caa + cbb
        L = np.empty(S.shape[:-1] + (2, 2))
        if model == "affine":
            det = caa * cbb - cab * cab
            ok = ok & (det > 1e-12 * (trc * trc))
            d = np.where(ok, det, 1.0)
            L[..., 0, 0] = (kax * cbb - kbx * cab) / d
            L[..., 0, 1] = (kbx * caa - kax * cab) / d
            L[..., 1, 0] = (kay * cbb - kby * cab) / d
            L[..., 1, 1] = (kby * caa - kay * cab) / d
        elif model == "translation":
            L[...] = np.eye(2)
        else:
            ok = ok & (trc > 0)
            tr, skew = kax + kby, kay - kbx
            if model == "similarity":
                d = np.where(ok, trc, 1.0)
                a, b = tr / d, skew / d
            else:
                ang = np.arctan2(skew, tr)
                a, b = np.cos(ang), np.sin(ang)
            L[..., 0, 0], L[..., 0, 1], L[..., 1, 0], L[..., 1, 1] = a, -b, b, a
        T = np.empty(S.shape[:-1] + (2, 3))
        T[..., :2] = L
        T[..., 0, 2] = mx - (L[..., 0, 0] * ma + L[..., 0, 1] * mb)
        T[..., 1, 2] = my - (L[..., 1, 0] * ma + L[..., 1, 1] * mb)
    T[~ok] = np.nan
    return T, ~ok


def _rms(sums):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((sums[..., 12] + sums[..., 13]) / np.where(sums[..., 0] > 0, sums[..., 0], np.nan))


def _fit_args(flow, model, weight, cell_size, trim, rounds):
    _check_model(model)
    flow_affine_moments_params(flow, weight, cell_size)
    if trim is not None:
        if isinstance(trim, bool) or not isinstance(trim, (int, float, np.integer, np.floating)) or not trim > 0:
            raise ValueError(f"trim must be a number > 0, got {trim!r}")
        trim = float(trim)
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or int(rounds) < 0:
        raise ValueError(f"rounds must be a non-negative integer, got {rounds!r}")
    return trim, int(rounds)


def fit_from_moments(moments, model="affine", trim=None, rounds=3):
    """The fit and its trim rounds over any source of moments: moments(prior, clip) -> (sums (14,), counts (4,)) of the
    whole image, prior a centred 2 x 3 matrix or None.  -> (centred matrix, counts per round, sums of the last round).
    ValueError if a fit is deficient."""
    def solve(sums):
        T, deficient = solve_flow_affine(sums, model)
        if deficient:
            raise ValueError(f"the {model!r} fit is rank deficient: no pixel of positive weight, or (other than for "
                             "\"translation\") sampling positions that do not span the model")
        return T
    sums, counts = moments(None, None)
    T, per_round = solve(sums), [tuple(int(v) for v in counts)]
    if trim is not None:
        for _ in range(rounds):
            sums, counts = moments(T, trim)
            T = solve(sums)
            per_round.append(tuple(int(v) for v in counts))
            if per_round[-1] == per_round[-2]:
                break
    return T, per_round, sums


def _total(ctx, flow, weight, cell_size, prior=None, clip=None):
    """the sums and counts of the whole image: with a per-cell weight, the cells' added up"""
    sums, counts = ctx.flow_affine_moments(flow, weight, cell_size, prior, clip)
    return sums.sum(axis=(0, 1)), counts.sum(axis=(0, 1))


def _fit(ctx, flow, model, weight, cell_size, trim, rounds):
    return fit_from_moments(lambda prior, clip: _total(ctx, flow, weight, cell_size, prior, clip), model, trim, rounds)


def fit_flow_affine(flow, model="affine", weight=None, cell_size=None, trim=None, rounds=3, return_info=False):
    """The 2 x 3 float64 matrix T, in Warper.tmat's convention and absolute pixel coordinates, that minimises
    sum w(p) |p - T (s(p), 1)|^2 over the (H, W, 2) float32 flow's sampling positions s(p) = p - flow(p): the global part
    of the flow.  split_flow(flow, T) is what it leaves.

    model: "affine" (6 parameters), "similarity" (rotation, one scale, shift), "rigid" (rotation, shift) or "translation".
    weight: what it is for smooth_flow -- None; an (H, W) float32 map or uint8 mask; or, with cell_size (an int or
    (cell_h, cell_w)), a (gy, gx) map on that cell grid (cell_size only gives the map's shape).  Non-finite pixels and
    pixels whose weight is NaN, negative or 0 take no part.
    trim: a residual in px.  The fit is made once untrimmed, then up to `rounds` times over the pixels whose residual
    against the previous matrix is within trim in x and in y; it stops early when the pixel counts repeat.  A loop, not a
    guarantee: a corrupted region that drags the first fit by more than trim takes good pixels out as well.
    ValueError if the fit is rank deficient, or if the image is more than 2^31 - 1 tiles of 510 x 64 pixels (sides of
    about 2^23 are the largest that one fit takes).  return_info: (tmat, FlowAffineInfo)."""
    weight = _cell_weight(weight, cell_size, getattr(_described(flow), "shape", ()))
    trim, rounds = _fit_args(_described(flow), model, weight, cell_size, trim, rounds)
    flow = dense_flow(flow)
    ctx = get_context()
    d_weight = None if weight is None else ctx.asdevice(weight)
    T, per_round, sums = _fit(ctx, ctx.asdevice(flow), model, d_weight, cell_size, trim, rounds)
    tmat = _to_absolute(T, flow.shape)
    return (tmat, FlowAffineInfo(per_round, float(_rms(sums)), model, T, None)) if return_info else tmat


def split_flow(flow, tmat=None, model="affine", weight=None, cell_size=None, trim=None, rounds=3, return_info=False):
    """(tmat, residual): the flow relative to the 2 x 3 matrix tmat, residual(p) = p - tmat (p - flow(p), 1), so that
    Warper(tmat=tmat, flow=residual) samples where Warper(flow=flow) does (up to rounding).  Without tmat it is fitted
    (fit_flow_affine with model, weight, cell_size, trim, rounds), which makes the residual the smallest in the weighted
    least-squares sense.  Non-finite pixels stay non-finite.  return_info: (tmat, residual, FlowAffineInfo), with the
    weighted RMS of the residual from a second pass over it."""
    like = _like(flow)
    weight = _cell_weight(weight, cell_size, getattr(_described(flow), "shape", ()))
    trim, rounds = _fit_args(_described(flow), model, weight, cell_size, trim, rounds)
    if tmat is not None:
        tmat = flow_affine_apply_params(_described(flow), tmat)[2].reshape(2, 3)
    flow = dense_flow(flow)
    ctx = get_context()
    d_flow = ctx.asdevice(flow)
    d_weight = None if weight is None else ctx.asdevice(weight)
    info = None
    if tmat is None:
        T, per_round, sums = _fit(ctx, d_flow, model, d_weight, cell_size, trim, rounds)
        tmat = _to_absolute(T, flow.shape)
        info = (per_round, float(_rms(sums)), model, T)
    elif return_info:
        sums, counts = _total(ctx, d_flow, d_weight, cell_size)
        info = ([tuple(int(v) for v in counts)], float(_rms(sums)), None, _to_centred(tmat, flow.shape))
    rest = ctx.flow_affine_apply(d_flow, tmat)
    out = rest if isinstance(like, DeviceArray) else rest.numpy()
    if not return_info:
        return tmat, out
    return tmat, out, FlowAffineInfo(*info, float(_rms(_total(ctx, rest, d_weight, cell_size)[0])))


def join_flow(tmat, flow):
    """The total flow of a matrix and a flow relative to it: F(p) = p - M (p - flow(p), 1), M = inv([tmat; 0 0 1]), so
    that Warper(flow=F) samples where Warper(tmat=tmat, flow=flow) does (up to rounding; without padding) -- the inverse
    of split_flow.  ValueError if [tmat; 0 0 1] is not invertible."""
    like = _like(flow)
    t = flow_affine_apply_params(_described(flow), tmat)[2].reshape(2, 3)
    det = t[0, 0] * t[1, 1] - t[0, 1] * t[1, 0]
    with np.errstate(all="ignore"):
        m = np.linalg.inv(np.append(t, [[0, 0, 1]], axis=0))[:2] if det != 0 else None
    if m is None or not np.all(np.isfinite(m)):
        raise ValueError(f"[tmat; 0 0 1] is not invertible: det = {det!r}")
    flow = dense_flow(flow)
    ctx = get_context()
    out = ctx.flow_affine_apply(ctx.asdevice(flow), m)
    return out if isinstance(like, DeviceArray) else out.numpy()


@dataclass
class FlowAffineMaps:
    """The affine part of a flow per cell (local_affine()); every map is (gy, gx), NaN where the cell is deficient."""
    cell_bounds: np.ndarray       # (gy, gx, 4) int64 of (y0, y1, x0, x1)
    model: str
    tmat: np.ndarray              # (gy, gx, 2, 3) float64, absolute pixel coordinates
    rotation_deg: np.ndarray      # atan2(T10 - T01, T00 + T11)
    scale: np.ndarray             # sqrt(|det L|): below 1 where the tissue shrank against the reference
    anisotropy: np.ndarray        # ratio of L's singular values, >= 1
    shift_x: np.ndarray           # T c - c at the cell's centre c, px
    shift_y: np.ndarray
    rms: np.ndarray               # weighted RMS of the flow over the cell's used pixels, px
    used: np.ndarray              # int64: pixels that took part
    deficient: np.ndarray         # bool: no fit (no weighted pixel, or positions that do not span the model)

    def summary(self) -> dict:
        """Median and extreme rotation, scale and shift over the cells that have a fit, and the most anisotropic cell."""
        ok = ~self.deficient
        out = {"cells": int(ok.size), "cells_deficient": int(self.deficient.sum()), "model": self.model}
        if not ok.any():
            out.update({"rotation_deg_median": float("nan"), "rotation_deg_range": None, "scale_median": float("nan"),
                        "scale_range": None, "shift_max": float("nan"), "anisotropy_max": float("nan"), "worst_cell": None,
                        "worst_cell_bounds": None})
            return out
        rot, sc = self.rotation_deg[ok], self.scale[ok]
        worst = np.unravel_index(int(np.argmax(np.where(ok, self.anisotropy, -1.0))), ok.shape)
        out.update({"rotation_deg_median": float(np.median(rot)), "rotation_deg_range": (float(rot.min()), float(rot.max())),
                    "scale_median": float(np.median(sc)), "scale_range": (float(sc.min()), float(sc.max())),
                    "shift_max": float(np.hypot(self.shift_x[ok], self.shift_y[ok]).max()),
                    "anisotropy_max": float(self.anisotropy[worst]), "worst_cell": tuple(int(i) for i in worst),
                    "worst_cell_bounds": tuple(int(v) for v in self.cell_bounds[worst])})
        return out


def affine_maps(sums, counts, shape, cell_size, model):
    """FlowAffineMaps from the per-cell sums (gy, gx, 14) and counts (gy, gx, 4) of an (H, W) flow: the host half of
    local_affine()."""
    from ..shared_modules.registration_qc import cell_bounds
    centred, deficient = solve_flow_affine(sums, model)
    tmat = _to_absolute(centred, shape)
    bounds = cell_bounds(shape, cell_size)
    if bounds.shape[:2] != tmat.shape[:2]:
        raise ValueError(f"sums of {tmat.shape[:2]} cells do not belong to cells {cell_size} of a {tuple(shape[:2])} flow")
    Lm = tmat[..., :2]
    cx, cy = (bounds[..., 2] + bounds[..., 3] - 1) / 2.0, (bounds[..., 0] + bounds[..., 1] - 1) / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        sv = np.linalg.svd(np.where(deficient[..., None, None], np.eye(2), Lm), compute_uv=False)
        aniso = np.where(deficient, np.nan, sv[..., 0] / sv[..., 1])
        det = Lm[..., 0, 0] * Lm[..., 1, 1] - Lm[..., 0, 1] * Lm[..., 1, 0]
        return FlowAffineMaps(
            cell_bounds=bounds, model=model, tmat=tmat,
            rotation_deg=np.degrees(np.arctan2(Lm[..., 1, 0] - Lm[..., 0, 1], Lm[..., 0, 0] + Lm[..., 1, 1])),
            scale=np.sqrt(np.abs(det)), anisotropy=aniso,
            shift_x=(Lm[..., 0, 0] * cx + Lm[..., 0, 1] * cy + tmat[..., 0, 2]) - cx,
            shift_y=(Lm[..., 1, 0] * cx + Lm[..., 1, 1] * cy + tmat[..., 1, 2]) - cy,
            rms=np.where(deficient, np.nan, _rms(np.asarray(sums, np.float64))), used=np.array(counts[..., 0], np.int64),
            deficient=deficient)


def local_affine(flow, cell_size, model="affine", weight=None):
    """What the tissue did, cell by cell: the fit of fit_flow_affine over each cell of the quality maps' grid (cells of
    cell_size, an int or (cell_h, cell_w), from (0, 0), the last row and column ragged) -> FlowAffineMaps with the matrix
    and its rotation, scale, anisotropy and shift at the cell's centre.  weight: None, an (H, W) float32 map or uint8
    mask, or a (gy, gx) map on the same grid.  A cell without a fit is flagged in `deficient` and NaN in the maps.  A cell
    holds at most 2^31 - 1 tiles of 510 x 64 pixels."""
    _check_model(model)
    if cell_size is None:
        raise ValueError("cell_size must be a positive integer or a pair of them, got None")
    weight = _cell_weight(weight, cell_size, getattr(_described(flow), "shape", ()))
    H, W, _, ch, cw, _, _ = flow_affine_moments_params(_described(flow), weight, cell_size)
    flow = dense_flow(flow)
    ctx = get_context()
    sums, counts = ctx.flow_affine_moments(ctx.asdevice(flow), None if weight is None else ctx.asdevice(weight), (ch, cw))
    return affine_maps(sums, counts, (H, W), (ch, cw), model)
