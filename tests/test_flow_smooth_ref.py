"""Smoothing, filling and unfolding flows on the CPU (no GPU): the numpy float32 statement of
include/microaligner_flowsmooth.h (tests/_flow_smooth_ref.py) against an independent float64 one, its identities, the fold
mask against a direct det J, the repair loop on a field that folds and has holes, and the argument checks of the entry
points before any device work."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_smooth_ref as R  # noqa: E402

F32, F64 = np.float32, np.float64


def noisy_flow(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    f = np.stack([3 * np.sin(x / 17) + 2 * np.cos(y / 23), 2.5 * np.cos(x / 13 + y / 31)], -1)
    return (f + rng.normal(0, 0.5, (H, W, 2))).astype(F32), rng


def holes(H, W, rng, r):
    """a keep mask with a few rectangular holes, each at least 2r + 1 away from the first rows and columns"""
    keep = np.ones((H, W), np.uint8)
    for _ in range(3):
        y0, x0 = int(rng.integers(H // 2, H)), int(rng.integers(W // 2, W))
        keep[y0:y0 + 9, x0:x0 + 14] = 0
    return keep


@pytest.mark.parametrize("sigma, r", [(1.0, 3), (8 / 3, 8), (7.0, 21), (20.0, 60)])
def test_statement_against_a_float64_one(sigma, r):
    """The float32 statement against scipy.ndimage.correlate1d(mode="constant") in float64 on w*u, w*v, w, with the same
    float32 taps, on 96 x 160 with weights that are 0 at 30 % of the pixels and 0.75 elsewhere.  Measured
    max |s32 - s64| / (2^-24 max|flow|) over three seeds: r = 3: 3.5 .. 4.5, r = 8: 4.2 .. 5.9, r = 21: 6.1 .. 6.5,
    r = 60: 7.6 .. 8.8 (seed 1, the one kept: 4.52, 5.90, 6.21, 8.85).  Bound: twice the worst case, rounded up to a
    power of two: 32 x 2^-24 max|flow|."""
    from scipy.ndimage import correlate1d
    f, rng = noisy_flow(96, 160, 1)
    w = (np.where(rng.random((96, 160)) < 0.3, 0, 1).astype(F32) * F32(0.75)).astype(F32)
    taps = R.gaussian_taps(sigma)
    assert len(taps) - 1 == r and abs(float(taps[0]) + 2 * float(taps[1:].astype(F64).sum()) - 1) < 1e-6
    s, unsupported = R.smooth_flow_ref(f, taps, w)
    assert unsupported == 0
    k = np.concatenate([taps[:0:-1], taps]).astype(F64)
    w64 = w.astype(F64)
    S = [correlate1d(correlate1d(p, k, axis=1, mode="constant"), k, axis=0, mode="constant")
         for p in (w64 * f[..., 0], w64 * f[..., 1], w64)]
    ref = np.stack([S[0] / S[2], S[1] / S[2]], -1)
    unit = 2.0 ** -24 * float(np.abs(f).max())
    err = float(np.abs(s.astype(F64) - ref).max()) / unit
    print(f"r = {r}: max |s32 - s64| = {err:.2f} x 2^-24 max|flow|")
    assert err <= 32


@pytest.mark.parametrize("kind", ["none", "f32", "u8", "cells"])
@pytest.mark.parametrize("mode", ["all", "blend"])
def test_a_constant_flow_comes_back_under_any_weights(kind, mode):
    H, W = 61, 83
    rng = np.random.default_rng(5)
    f = np.empty((H, W, 2), F32)
    f[...] = (3.25, -1234.5)
    weight, cells = None, None
    if kind == "f32":
        weight = rng.uniform(0, 3, (H, W)).astype(F32)
        weight[rng.random((H, W)) < 0.4] = 0
    elif kind == "u8":
        weight = (rng.random((H, W)) < 0.5).astype(np.uint8) * 200
    elif kind == "cells":
        cells = (16, 48)
        weight = rng.uniform(0.5, 2, (4, 2)).astype(F32)
        weight[1, 0] = 0
    out, unsupported = R.smooth_flow_ref(f, R.gaussian_taps(4.0), weight, cells, mode)
    assert unsupported == 0
    assert np.abs(out / f - 1).max() <= 1e-5


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (7, 5), (70, 90)])
@pytest.mark.parametrize("r_sigma", [1 / 3, 2.0, 40.0])
def test_blend_with_no_dropped_pixel_returns_the_input_bit_for_bit(shape, r_sigma):
    f, rng = noisy_flow(*shape, 7)
    f[0, 0] = (1e30, -1e-30)
    taps = R.gaussian_taps(r_sigma)
    # (a uniform weight below 3/4 would lower c below the point where a == 1: the feathering reads it as partly dropped)
    for weight in (None, np.ones(shape, np.uint8), np.ones(shape, F32), np.full(shape, 2.5, F32)):
        out, unsupported = R.smooth_flow_ref(f, taps, weight, None, "blend")
        assert unsupported == 0 and np.array_equal(out.view(np.uint32), f.view(np.uint32))


@pytest.mark.parametrize("sigma", [2.0, 3.0, 7.0])      # r = 6, 9, 21: every pixel of the 9 x 14 holes has support
def test_pixels_with_no_dropped_pixel_within_r_are_bit_identical(sigma):
    H, W = 120, 150
    f, rng = noisy_flow(H, W, 11)
    taps = R.gaussian_taps(sigma)
    r = len(taps) - 1
    keep = holes(H, W, rng, r)
    f[~keep.astype(bool)] = np.nan
    f[5, 7] = np.inf                                    # dropped by its value, not by the mask
    dropped = ~(keep.astype(bool) & np.isfinite(f).all(-1))
    marks = np.zeros((H, W, 2), F32)
    marks[dropped] = np.nan
    near = R.fold_mask_ref(marks, r)[0] == 0             # within r (Chebyshev) of a dropped pixel
    assert 0 < near.mean() < 0.6
    out, unsupported = R.smooth_flow_ref(f, taps, keep, None, "blend")
    assert np.array_equal(out[~near].view(np.uint32), f[~near].view(np.uint32))
    assert unsupported == 0 and np.isfinite(out).all()
    # and the filled values join the rim: no step larger than the field's own across a hole's edge
    step = max(float(np.abs(np.diff(out, axis=0)).max()), float(np.abs(np.diff(out, axis=1)).max()))
    inside = np.isfinite(f).all(-1)
    own = max(float(np.abs(np.diff(f, axis=0))[inside[1:] & inside[:-1]].max()),
              float(np.abs(np.diff(f, axis=1))[inside[:, 1:] & inside[:, :-1]].max()))
    assert step <= own


def direct_det(f):
    """det J written out pixel by pixel in float64: central differences inside, one-sided at the edges"""
    H, W = f.shape[:2]
    u, v = f[..., 0].astype(F64), f[..., 1].astype(F64)
    det = np.empty((H, W))
    with np.errstate(all="ignore"):
        for y in range(H):
            ym, yp = max(y - 1, 0), min(y + 1, H - 1)
            for x in range(W):
                xm, xp = max(x - 1, 0), min(x + 1, W - 1)
                dx, dy = max(xp - xm, 1), max(yp - ym, 1)
                det[y, x] = (1 + (u[y, xp] - u[y, xm]) / dx) * (1 + (v[yp, x] - v[ym, x]) / dy) \
                    - ((u[yp, x] - u[ym, x]) / dy) * ((v[y, xp] - v[y, xm]) / dx)
    return det


@pytest.mark.parametrize("shape", [(96, 160), (1, 40), (40, 1), (1, 1), (2, 2)])
def test_fold_mask_counts_equal_a_direct_det_j(shape):
    f = R.repair_case()[:shape[0], :shape[1]] if shape != (96, 160) else R.repair_case()
    f = np.ascontiguousarray(f)
    det = direct_det(f)
    with np.errstate(all="ignore"):
        folded = int((np.isfinite(det) & (det <= 0)).sum())
    invalid = int((~np.isfinite(f).all(-1)).sum())
    for margin in (0, 2):
        keep, counts = R.fold_mask_ref(f, margin)
        assert counts[:2] == (folded, invalid) and counts[2] == int((keep == 0).sum())
        assert keep.dtype == np.uint8 and set(np.unique(keep)) <= {0, 1}
    if shape == (96, 160):
        assert (folded, invalid) == (105, 1768)
        keep0 = R.fold_mask_ref(f, 0)[0]
        assert not keep0[0, 0] and not keep0[95, 157:].any() and not keep0[20:62, 58:100].any()


@pytest.mark.parametrize("sigma, margin, most", [(6.0, 4, 3), (4.0, 2, 4)])
def test_repair_loop_converges_on_the_test_field(sigma, margin, most):
    """Measured: 2 smoothing rounds with (6.0, 4), 3 with (4.0, 2)."""
    f = R.repair_case()
    assert R.fold_mask_ref(f, 0)[1][:2] == (105, 1768)
    out, rounds, converged, _ = R.repair_flow_ref(f, sigma, margin)
    print(sigma, margin, rounds)
    assert converged and 1 <= len(rounds) <= most
    assert np.isfinite(out).all()
    assert R.fold_mask_ref(out, 0)[1][:2] == (0, 0) and float(R.det_j(out).min()) > 0
    assert rounds[0][:2] == (105, 1768)


def test_repair_loop_is_no_guarantee():
    """sigma <= 3 stalls on this field: a kernel that is small against the folds smooths one away and leaves another beside
    it, round after round.  The loop reports it; it does not promise a fold-free flow."""
    for sigma in (3.0, 2.0):
        out, rounds, converged, _ = R.repair_flow_ref(R.repair_case(), sigma, 2)
        assert not converged and len(rounds) == 8 and R.fold_mask_ref(out, 0)[1][0] > 0


# ---- argument checks before any device work ------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import microaligner_amd.device as dev
    import microaligner_amd.optflow_reg.flow_smooth as mod

    def refuse(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(mod, "get_context", refuse)
    monkeypatch.setattr(dev, "get_context", refuse)


FLOW = np.zeros((8, 9, 2), F32)


@pytest.mark.parametrize("kw", [
    dict(flow=FLOW.astype(F64)), dict(flow=FLOW[..., 0]), dict(flow=np.zeros((0, 9, 2), F32)), dict(flow=[[0.0, 0.0]]),
    dict(sigma=0), dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.inf), dict(sigma="6"), dict(sigma=None), dict(sigma=True),
    dict(sigma=43.0), dict(sigma=6.0, truncate=22.0), dict(truncate=0), dict(truncate=np.nan),
    dict(where="ALL"), dict(where="mix"), dict(where=None), dict(where=1),
    dict(min_support=-1e-3), dict(min_support=np.nan), dict(min_support=np.inf), dict(min_support=1e39), dict(min_support="0"),
    dict(weight=np.ones((8, 9), F64)), dict(weight=np.ones((8, 8), F32)), dict(weight=np.ones((8, 9, 2), F32)),
    dict(weight=np.ones((8, 9), bool)), dict(weight=[[1.0]]), dict(cell_size=4),
    dict(weight=np.ones((2, 3), F32), cell_size=3), dict(weight=np.ones((2, 3), F32), cell_size=(4, 5)),
    dict(weight=np.ones((2, 3), F32), cell_size=0), dict(weight=np.ones((2, 3), F32), cell_size=(4, 0)),
    dict(weight=np.ones((2, 3), F32), cell_size=(4, 3, 2)), dict(weight=np.ones((2, 3), F32), cell_size=2.5),
    dict(weight=np.ones((2, 3), "U1"), cell_size=(4, 3))])
def test_smooth_flow_refuses_bad_arguments_before_device_work(no_device, kw):
    from microaligner_amd import smooth_flow
    with pytest.raises(ValueError):
        smooth_flow(**dict(dict(flow=FLOW, sigma=2.0), **kw))


@pytest.mark.parametrize("kw", [dict(flow=FLOW.astype(F64)), dict(flow=FLOW[..., 0]), dict(margin=-1), dict(margin=33),
                                dict(margin=2.0), dict(margin=True), dict(margin=None)])
def test_fold_mask_and_repair_flow_refuse_bad_arguments_before_device_work(no_device, kw):
    from microaligner_amd import fold_mask, repair_flow
    with pytest.raises(ValueError):
        fold_mask(**dict(dict(flow=FLOW), **kw))
    with pytest.raises(ValueError):
        repair_flow(**dict(dict(flow=FLOW), **kw))


@pytest.mark.parametrize("kw", [dict(sigma=0.0), dict(sigma=43.0), dict(sigma=None), dict(max_rounds=-1), dict(max_rounds=2.0),
                                dict(max_rounds=True)])
def test_repair_flow_refuses_bad_arguments_before_device_work(no_device, kw):
    from microaligner_amd import repair_flow
    with pytest.raises(ValueError):
        repair_flow(**dict(dict(flow=FLOW), **kw))


def test_taps_of_the_package_are_the_statements():
    from microaligner_amd.device import gaussian_taps
    for sigma, truncate in ((6.0, 3.0), (0.2, 3.0), (1.0, 3.0), (42.0, 3.0), (4.0, 2.5), (128.0, 1.0)):
        a, b = gaussian_taps(sigma, truncate), R.gaussian_taps(sigma, truncate)
        assert a.dtype == F32 and np.array_equal(a, b)
    assert len(gaussian_taps(6.0)) == 19 and len(gaussian_taps(0.2)) == 2 and len(gaussian_taps(128 / 3)) == 129
