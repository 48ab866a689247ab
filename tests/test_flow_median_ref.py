"""Median-filtering a flow on the CPU (no GPU): the numpy statement of include/microaligner_flowmedian.h
(tests/_flow_median_ref.py) against scipy's median filter and a pure-Python sort, its identities (ramps, edges, signed
zeros, denormals), and the argument checks of the entry points before any device work."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_median_ref as R  # noqa: E402

F32, F64 = np.float32, np.float64
FLT_MAX = np.finfo(F32).max


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def noisy(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 3, (H, W, 2)).astype(F32), rng


@pytest.mark.parametrize("r", [1, 2, 3, 4, 7])
def test_interior_equals_scipys_median_filter(r):
    from scipy.ndimage import median_filter
    f, _ = noisy(40, 53, r)
    out, keep, counts = R.median_flow_ref(f, r)
    for c in range(2):
        ref = median_filter(f[..., c], size=2 * r + 1, mode="constant")
        assert np.array_equal(bits(out[r:-r, r:-r, c]), bits(ref[r:-r, r:-r]))
    assert keep.all() and counts == (0, 0, 0)


def python_median(f, part, r, x, y, c):
    H, W = part.shape
    vals = [f[yy, xx, c] for yy in range(max(0, y - r), min(H, y + r + 1)) for xx in range(max(0, x - r), min(W, x + r + 1))
            if part[yy, xx]]
    return sorted(vals)[(len(vals) - 1) // 2] if vals else None


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (4, 5), (7, 5), (12, 17)])
@pytest.mark.parametrize("r", [1, 2, 7])
@pytest.mark.parametrize("kind", ["none", "u8", "f32", "cells"])
def test_borders_and_masks_equal_a_python_sort(shape, r, kind):
    H, W = shape
    f, rng = noisy(H, W, 7 * H + W + r)
    if H * W > 6:
        f[H // 2, W // 2] = (np.nan, 1.0)
        f[0, W - 1] = (2.0, np.inf)
    weight, cells = None, None
    if kind == "u8":
        weight = (rng.random(shape) < 0.6).astype(np.uint8) * 7
    elif kind == "f32":
        weight = rng.uniform(-1, 2, shape).astype(F32)
        weight[0, 0] = np.nan
        weight[-1, -1] = np.inf
    elif kind == "cells":
        cells = (3, 4)
        weight = (rng.random((-(-H // 3), -(-W // 4))) < 0.6).astype(F32)
    out, keep, counts = R.median_flow_ref(f, r, weight, cells, "outliers", 0.5)
    part = R.participates(f, weight, cells)
    expected_part = np.ones(shape, bool)
    for y in range(H):
        for x in range(W):
            wv = 1.0 if weight is None else float(weight[y // 3, x // 4]) if cells else float(weight[y, x])
            expected_part[y, x] = np.isfinite(wv) and wv > 0 and bool(np.isfinite(f[y, x]).all())
    assert np.array_equal(part, expected_part)
    n_out = n_drop = n_uns = 0
    for y in range(H):
        for x in range(W):
            m = [python_median(f, part, r, x, y, c) for c in range(2)]
            if m[0] is None:
                assert np.isnan(out[y, x]).all() and keep[y, x] == 0 and not part[y, x]
                n_uns += 1
                n_drop += 1
                continue
            m = np.array(m, F32)
            if not part[y, x]:
                n_drop += 1
                exp, k = m, 0
            else:
                d = max(abs(F32(f[y, x, 0] - m[0])), abs(F32(f[y, x, 1] - m[1])))
                k = 0 if d > F32(0.5) else 1
                n_out += 1 - k
                exp = f[y, x] if k else m
            assert np.array_equal(bits(out[y, x]), bits(exp)) and keep[y, x] == k
    assert counts == (n_out, n_drop, n_uns)
    # where="all" gives the medians themselves, and the same keep and counts
    out_all, keep_all, counts_all = R.median_flow_ref(f, r, weight, cells, "all", 0.5)
    assert np.array_equal(keep_all, keep) and counts_all == counts
    same = (keep == 0) & ~np.isnan(out).any(-1)
    assert np.array_equal(bits(out_all[same]), bits(out[same]))


@pytest.mark.parametrize("r", [1, 2, 5])
def test_a_float32_ramp_comes_back_bit_for_bit_in_the_interior(r):
    """u = fl(a x + b y + c): rounding is monotone, so it commutes with the median of an odd window, and the median of
    the exact ramp over a window centred at p is its value at p"""
    y, x = np.mgrid[0:31, 0:45].astype(F64)
    f = np.stack([0.37 * x - 1.21 * y + 3.3, -0.011 * x + 0.5 * y - 100.7], -1).astype(F32)
    out, keep, counts = R.median_flow_ref(f, r, None, None, "all", 0.0)
    assert np.array_equal(bits(out[r:-r, r:-r]), bits(f[r:-r, r:-r]))
    assert keep[r:-r, r:-r].all() and counts[1:] == (0, 0)


def test_a_vertical_step_edge_stays_where_it_is():
    f = np.zeros((20, 30, 2), F32)
    f[:, 15:] = (5.0, -3.0)
    for r in (1, 2, 7):
        out, keep, counts = R.median_flow_ref(f, r, None, None, "all", 0.0)
        assert np.array_equal(bits(out), bits(f)) and keep.all() and counts == (0, 0, 0)


def test_signed_zeros_denormals_and_flt_max_are_ordered_and_survive():
    vals = np.array([-FLT_MAX, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1e-40, 1.0, FLT_MAX], F32)
    k = R.keys(vals)
    assert k.dtype == np.int32 and np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(bits(R.values(k)), bits(vals))
    allbits = np.arange(-2 ** 31, 2 ** 31, 2 ** 16 + 1, dtype=np.int64).astype(np.int32).view(F32)
    assert np.array_equal(bits(R.values(R.keys(allbits))), bits(allbits))
    nan_keys = R.keys(np.array([0xffffffff, 0x7fffffff], np.uint32).view(F32))
    assert list(nan_keys) == [-2 ** 31, 2 ** 31 - 1]                  # the sentinels are NaNs' keys
    finite = R.keys(np.array([-FLT_MAX, FLT_MAX], F32))
    assert -2 ** 31 < finite[0] and finite[1] < 2 ** 31 - 1
    # a 3 x 3 image is one window for its centre: the median of the nine values is the middle one, whatever the layout
    rng = np.random.default_rng(3)
    for _ in range(20):
        f = np.stack([rng.permutation(vals), rng.permutation(vals)], -1).reshape(3, 3, 2)
        out, _, _ = R.median_flow_ref(f, 1)
        assert np.array_equal(bits(out[1, 1]), bits(np.array([0.0, 0.0], F32)))
    f = np.zeros((3, 3, 2), F32)
    f[..., 0].flat[:5] = -0.0                        # five -0.0 and four +0.0: the median is -0.0
    f[..., 1].flat[:4] = -0.0                        # four -0.0 and five +0.0: +0.0
    out, _, _ = R.median_flow_ref(f, 1)
    assert np.array_equal(bits(out[1, 1]), bits(np.array([-0.0, 0.0], F32)))
    # FLT_MAX against -FLT_MAX: the distance overflows to +Inf, an outlier for every finite thresh and none for +Inf
    f = np.full((3, 3, 2), -FLT_MAX, F32)
    f[1, 1] = FLT_MAX
    assert R.median_flow_ref(f, 1, None, None, "all", 1e30)[2][0] == 1
    assert R.median_flow_ref(f, 1, None, None, "all", np.inf)[2][0] == 0


def test_the_effect_on_a_spiked_flow():
    """fewer spikes than half of every window: each spike returns to within r (Lx + Ly) of the clean flow, nothing else moves"""
    clean, spiked, spikes, Lx, Ly = R.spiked_flow()
    r = 2
    cnt, size = R.window_count(spikes, r)
    assert spikes.sum() > 50 and np.all(2 * cnt < size)
    bound = r * (Lx + Ly)
    thresh = F32(1.01 * bound)
    assert 20 - bound > thresh
    out, keep, counts = R.median_flow_ref(spiked, r, None, None, "outliers", thresh)
    assert np.abs(out.astype(F64) - clean)[spikes].max() <= bound
    assert np.array_equal(bits(out[~spikes]), bits(spiked[~spikes]))
    assert counts == (int(spikes.sum()), 0, 0) and np.array_equal(keep == 0, spikes)


# ---- argument checks before any device work ------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import microaligner_amd.device as dev
    import microaligner_amd.optflow_reg.flow_median as mod

    def refuse(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(mod, "get_context", refuse)
    monkeypatch.setattr(dev, "get_context", refuse)


FLOW = np.zeros((8, 9, 2), F32)
BAD = [
    dict(flow=FLOW.astype(F64)), dict(flow=FLOW[..., 0]), dict(flow=np.zeros((0, 9, 2), F32)), dict(flow=[[0.0, 0.0]]),
    dict(radius=0), dict(radius=8), dict(radius=-1), dict(radius=2.0), dict(radius=True), dict(radius=None), dict(radius="2"),
    dict(thresh=-1.0), dict(thresh=np.nan), dict(thresh="1"), dict(thresh=True),
    dict(weight=np.ones((8, 9), F64)), dict(weight=np.ones((8, 8), F32)), dict(weight=np.ones((8, 9, 2), F32)),
    dict(weight=np.ones((8, 9), bool)), dict(weight=[[1.0]]), dict(cell_size=4),
    dict(weight=np.ones((2, 3), F32), cell_size=3), dict(weight=np.ones((2, 3), F32), cell_size=(4, 5)),
    dict(weight=np.ones((2, 3), F32), cell_size=0), dict(weight=np.ones((2, 3), F32), cell_size=(4, 0)),
    dict(weight=np.ones((2, 3), F32), cell_size=(4, 3, 2)), dict(weight=np.ones((2, 3), F32), cell_size=2.5),
    dict(weight=np.ones((2, 3), "U1"), cell_size=(4, 3))]


@pytest.mark.parametrize("kw", BAD + [dict(where="ALL"), dict(where="blend"), dict(where=None), dict(where=1),
                                      dict(where="outliers"), dict(where="outliers", thresh=None)])
def test_median_flow_refuses_bad_arguments_before_device_work(no_device, kw):
    from microaligner_amd import median_flow
    with pytest.raises(ValueError):
        median_flow(**dict(dict(flow=FLOW), **kw))


@pytest.mark.parametrize("kw", BAD + [dict(thresh=None)])
def test_outlier_mask_refuses_bad_arguments_before_device_work(no_device, kw):
    from microaligner_amd import outlier_mask
    with pytest.raises(ValueError):
        outlier_mask(**dict(dict(flow=FLOW), **kw))


def test_params_of_the_package():
    from microaligner_amd import _lib
    from microaligner_amd.device import median_flow_params
    assert median_flow_params(FLOW) == (8, 9, 2, _lib.MA_SMOOTH_WEIGHT_NONE, 1, 1, _lib.MA_MEDIAN_ALL, float("inf"), 0)
    got = median_flow_params(FLOW, 7, np.ones((2, 3), F32), (4, 3), "outliers", 0, True)
    assert got == (8, 9, 7, _lib.MA_SMOOTH_WEIGHT_CELLS, 4, 3, _lib.MA_MEDIAN_OUTLIERS, 0.0, _lib.MA_MEDIAN_GENERIC)
    assert median_flow_params(FLOW, 1, np.ones((8, 9), np.uint8), None, "all", np.inf)[3] == _lib.MA_SMOOTH_WEIGHT_U8
    assert median_flow_params(FLOW, 1, thresh=1e39)[7] == float("inf")       # rounds to +Inf as float32: "none"
    assert _lib.MA_MEDIAN_MAX_RADIUS == R.MAX_RADIUS == 7
    with pytest.raises(ValueError):
        median_flow_params(FLOW, generic=1)
    # the grid of tiles: sides within [1, 2^24] whose 32 x 64 tiles number more than 2^31 - 1 are refused as the C entry does
    from types import SimpleNamespace
    side = 1 << 24
    with pytest.raises(ValueError, match="too large"):
        median_flow_params(SimpleNamespace(shape=(side, side, 2), dtype=np.dtype(F32)))
    assert median_flow_params(SimpleNamespace(shape=(side, 8191, 2), dtype=np.dtype(F32)))[:2] == (side, 8191)
