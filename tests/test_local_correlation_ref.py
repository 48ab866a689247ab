"""The local correlation maps without a device: the numpy float32 statement of include/microaligner_localcorr.h
(tests/_local_correlation_ref.py) against a float64 one, what the map says on a pair with a known defect, the argument
checks of local_correlation_params() and local_correlation(), and the plumbing of the new header."""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_smooth_ref as S  # noqa: E402
import _local_correlation_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_localcorr.h")
DTYPES = [np.uint8, np.uint16, np.float32]
# |s32 - s64| <= K 2^-24 (Maa / (va + floor) + Mbb / (vb + floor) + 1): the second moments about the centres over the
# regularised variances say how much of the sums cancels.  Measured with this statement over the 36 cases of
# test_statement_against_a_float64_one: K from 3.1 to 9.3 centred and from 3.5 to 9.9 uncentred; 4 times the largest is allowed.
K_MEASURED, K_ALLOWED = 9.93, 40.0


def taps_of(r):
    sigma = r / 3.0
    taps = S.gaussian_taps(sigma, (r - 0.5) / sigma)         # ceil(r - 0.5) = r whatever the rounding of the product
    assert len(taps) == r + 1
    return taps


def medians(ref, img):
    return float(F32(np.median(ref))), float(F32(np.median(img)))


def bound(m64, floor, k=K_ALLOWED):
    return k * 2.0 ** -24 * (m64["Maa"] / (m64["va"] + floor) + m64["Mbb"] / (m64["vb"] + floor) + 1)


@functools.lru_cache(maxsize=None)
def both(shape, dtype, r, centred):
    """(float32 statement, float64 statement, floor) of the pair; floor = 4 x the noise variance"""
    ref, img, nv = R.pair(*shape, dtype)
    c = medians(ref, img) if centred else (0.0, 0.0)
    return R.local_correlation_ref(ref, img, taps_of(r), 4 * nv, c), R.local_correlation_f64(ref, img, taps_of(r), 4 * nv, c), 4 * nv


@pytest.mark.parametrize("centred", [True, False])
@pytest.mark.parametrize("r", [3, 12, 49])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(96, 161), (37, 515)])
def test_statement_against_a_float64_one(shape, dtype, r, centred):
    m32, m64, floor = both(shape, dtype, r, centred)
    err = np.abs(m32["score"].astype(F64) - m64["score"])
    k = float((err / bound(m64, floor, 1.0)).max())
    print(f"{shape} {np.dtype(dtype).name} r={r} centred={centred}: K = {k:.2f}, largest |s32 - s64| = {err.max():.3g}")
    assert np.isfinite(m64["score"]).all() and (err <= bound(m64, floor)).all()


@pytest.mark.parametrize("r", [3, 12, 49])
def test_centring_by_the_median_is_the_more_accurate_on_uint16(r):
    """measured at r = 3 / 12 / 49: 4.4e-5 / 5.8e-5 / 9.8e-5 centred against 5.2e-4 / 7.1e-4 / 1.3e-3 uncentred"""
    err = []
    for centred in (True, False):
        m32, m64, _ = both((96, 161), np.uint16, r, centred)
        err.append(float(np.abs(m32["score"].astype(F64) - m64["score"]).max()))
    print(f"r={r}: centred {err[0]:.3g}, uncentred {err[1]:.3g}")
    assert err[0] < err[1]


@pytest.mark.parametrize("sigma", [1.0, 4.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_map_says_what_it_should(dtype, sigma):
    """measured medians at sigma 1 / 4 (uint16): 0.966 / 0.994 on the texture, -0.79 / -0.34 in the block's core, |s| 0.03 /
    0.009 on the constant part"""
    H, W = 96, 161
    ref, img, nv = R.pair(H, W, dtype)
    taps = S.gaussian_taps(sigma)
    m = R.local_correlation_ref(ref, img, taps, 4 * nv, medians(ref, img), cell_size=(32, 80))
    tex, blk, flat = R.regions(H, W, len(taps) - 1)
    s, cls = m["score"], m["classes"]
    print(f"{np.dtype(dtype).name} sigma={sigma}: texture {np.median(s[tex]):.3f}, block {np.median(s[blk]):.3f}, "
          f"constant |s| {np.median(np.abs(s[flat])):.4f}")
    assert tex.sum() > 1000 and blk.sum() > 100 and flat.sum() > 1000
    assert (cls[tex] == R.AGREE).all() and (s[tex] >= 0.75).all() and (m["weight"][tex] == 1).all()
    assert (s[blk] < 0.25).all() and not m["weight"][blk].any() and (cls[blk] == R.DISAGREE).all()
    assert (cls[flat] == R.FLAT).all()
    assert not (cls == R.UNSUPPORTED).any()
    assert np.array_equal(m["counts"].sum(-1), R.cell_counts(np.zeros((H, W), np.uint8), (32, 80), 1)[..., 0])
    assert m["counts"].shape == (3, 3, 4) and m["counts"][..., R.DISAGREE].argmax() == 3      # the block's cell: (1, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_score_is_blind_to_bias_and_to_gain_up_to_the_floor(dtype):
    """The other image b becomes g b + o.  Mathematically a bias o leaves every term as it is, and a gain g turns
    vb + floor into g^2 (vb + floor / g^2): the score is multiplied by sqrt((vb + floor) / (vb + floor / g^2)) -- the
    blindness to gain is exact only as far as the floor is small against vb -- and by nothing else.  Each float32 score
    is within the bound of test_statement_against_a_float64_one of its exact value, so two of them differ by less than the
    sum of their bounds once that factor is taken out."""
    H, W, r = 96, 161, 12
    ref, img, nv = R.pair(H, W, dtype)
    floor, taps = 4 * nv, taps_of(r)
    base32 = R.local_correlation_ref(ref, img, taps, floor, medians(ref, img))["score"].astype(F64)
    base64 = R.local_correlation_f64(ref, img, taps, floor, medians(ref, img))
    for g, o in ((1.0, 0.21), (1.0, -0.4), (1.7, 0.0), (0.45, 0.13)):
        other = (g * img.astype(F64) + o * R.full_scale(dtype)).astype(F32)
        c = medians(ref, other)
        got = R.local_correlation_ref(ref, other, taps, floor, c)["score"].astype(F64)
        m64 = R.local_correlation_f64(ref, other, taps, floor, c)
        factor = np.sqrt((base64["vb"] + floor) / (base64["vb"] + floor / g ** 2))
        moved = np.abs(got - base32 * factor)
        print(f"{np.dtype(dtype).name} gain {g} bias {o}: the score moves by {moved.max():.3g} at most")
        assert (moved <= bound(base64, floor) + bound(m64, floor)).all()


def test_weights_masks_and_support():
    """a pixel outside the mask takes no part; a window without live pixels is unsupported, weight 0; the counts sum to
    each cell's size"""
    H, W, r = 40, 70, 3
    ref, img, nv = R.pair(H, W, np.uint8, block=False)
    mask = np.ones((H, W), np.uint8)
    mask[:, 20:40] = 0
    ref2, img2 = ref.copy(), img.copy()
    ref2[:, 20:40], img2[:, 20:40] = 255, -7.0
    a = R.local_correlation_ref(ref, img, taps_of(r), 4 * nv, weight=mask, cell_size=(16, 48))
    b = R.local_correlation_ref(ref2, img2, taps_of(r), 4 * nv, weight=mask, cell_size=(16, 48))
    assert np.array_equal(a["score"], b["score"], equal_nan=True)
    dead = np.isnan(a["score"])
    assert dead[:, 20 + r:40 - r].all() and not dead[:, :20].any() and not dead[:, 40:].any()
    assert not a["weight"][dead].any() and (a["classes"][dead] == R.UNSUPPORTED).all()
    assert a["counts"].shape == (3, 2, 4) and a["counts"].sum() == H * W and a["counts"][0, 0].sum() == 16 * 48
    w = np.where(mask, F32(0.37), F32(np.nan)).astype(F32)
    w[0, 0], w[1, 1], w[2, 2] = -1.0, 0.0, np.inf
    c = R.local_correlation_ref(ref, img, taps_of(r), 4 * nv, weight=w, min_support=0.2)
    assert np.isnan(c["score"][0, 0]) and np.isfinite(c["score"][20, 60])       # the corner's window holds about 0.37 / 2
    # a NaN or Inf pixel of either image is dropped like a masked one
    img3 = img.copy()
    img3[5, 5], img3[30, 60] = np.nan, np.inf
    m3 = np.ones((H, W), np.uint8)
    m3[5, 5] = m3[30, 60] = 0
    assert np.array_equal(R.local_correlation_ref(ref, img3, taps_of(r), 4 * nv)["score"],
                          R.local_correlation_ref(ref, img, taps_of(r), 4 * nv, weight=m3)["score"])


# ---- argument checks -------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_c_entry_raises_before_any_device_work():
    from microaligner_amd import device
    from microaligner_amd.device import local_correlation_params as P
    ref, img = np.zeros((20, 30), np.uint8), np.zeros((20, 30), F32)
    taps = taps_of(3)
    H, W, dtype, t, r, center, floor, kind, ms, lo, hi, ch, cw, want = P(ref, img, taps, 2.5)
    assert (H, W, dtype, r, center, floor, kind, ms, lo, hi, ch, cw, want) == \
        (20, 30, 0, 3, (0.0, 0.0), 2.5, 0, 0.0, 0.25, 0.75, None, None, ("score",))
    got = P(ref.astype(np.uint16), img, taps, 1e-3, (3, -4.5), np.ones((20, 30), np.uint8), -1, 1, 0.5, 7, ("weight", "score"))
    assert got[2] == 1 and got[5] == (3.0, -4.5) and got[7:] == (2, 0.5, -1.0, 1.0, 7, 7, ("weight", "score"))
    assert P(ref.astype(F32), img, taps, 1.0, weight=np.ones((20, 30), F32), cell_size=(4, 9), want=())[7:] == \
        (1, 0.0, 0.25, 0.75, 4, 9, ())
    ok = dict(ref=ref, img=img, taps=taps, floor=1.0)
    for bad in (dict(ref=None), dict(ref=[[1, 2]]), dict(ref=np.zeros((4, 5, 2), np.uint8)), dict(ref=np.zeros(7, np.uint8)),
                dict(ref=np.zeros((20, 30), F64)), dict(ref=np.zeros((20, 30), np.int16)), dict(ref=np.zeros((20, 31), np.uint8)),
                dict(ref=np.zeros((0, 30), np.uint8), img=np.zeros((0, 30), F32)),
                dict(img=None), dict(img=np.zeros((20, 30), np.uint8)), dict(img=np.zeros((20, 30), F64)),
                dict(img=np.zeros((30, 20), F32)), dict(img=np.zeros((20, 30, 1), F32)),
                dict(taps=None), dict(taps=list(taps)), dict(taps=taps.astype(F64)), dict(taps=taps[:1]),
                dict(taps=np.ones(130, F32)), dict(taps=np.zeros(4, F32)), dict(taps=-taps),
                dict(taps=np.array([0.5, np.nan], F32)), dict(taps=np.array([0.0, 0.5], F32)),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=1e-50),
                dict(floor=1e40), dict(floor="1"), dict(floor=True), dict(floor=None),
                dict(center=None), dict(center="median"), dict(center=1.0), dict(center=(1.0,)), dict(center=(1, 2, 3)),
                dict(center=(float("nan"), 0)), dict(center=(0, float("inf"))), dict(center=(0, 1e40)), dict(center=("0", 0)),
                dict(lo=0.75), dict(lo=0.8), dict(hi=0.25), dict(lo=-1.01), dict(hi=1.01), dict(lo=float("nan")),
                dict(hi=float("nan")), dict(lo=0.5, hi=0.5 + 1e-9), dict(lo="0"), dict(hi=None),
                dict(min_support=-0.1), dict(min_support=float("nan")), dict(min_support=float("inf")), dict(min_support="0"),
                dict(weight=[[1.0]]), dict(weight=np.ones((20, 30), F64)), dict(weight=np.ones((20, 31), F32)),
                dict(weight=np.ones((20, 30), bool)), dict(weight=np.ones((2, 2), F32), cell_size=10),
                dict(want=()), dict(want="score"), dict(want=("score", "score")), dict(want=("s",)), dict(want=(1,)),
                dict(cell_size=0), dict(cell_size=(4, 0)), dict(cell_size=(-1, 4)), dict(cell_size=2.5), dict(cell_size=(1, 2, 3))):
        with pytest.raises(ValueError):
            P(**dict(ok, **bad))
    big, bimg = object.__new__(device.DeviceArray), object.__new__(device.DeviceArray)      # sides are checked on the shape alone
    for shape in (((1 << 24) + 1, 2), (2, (1 << 24) + 1)):
        big.shape, big.dtype, bimg.shape, bimg.dtype = shape, np.dtype(np.uint8), shape, np.dtype(F32)
        with pytest.raises(ValueError):
            P(big, bimg, taps, 1.0)
    big.shape = bimg.shape = (1 << 24, 1 << 24)
    assert P(big, bimg, taps, 1.0)[:2] == (1 << 24, 1 << 24)
    big.ptr = big.ctx = bimg.ptr = bimg.ctx = None             # nothing for __del__ to free


def test_local_correlation_refuses_its_own_arguments_before_any_device_work(monkeypatch):
    from microaligner_amd.shared_modules import local_correlation as M
    monkeypatch.setattr(M, "get_context", lambda: pytest.fail("a refused call reached the device"))
    ref, mov = np.zeros((20, 30), np.uint8), np.zeros((20, 30), np.uint16)
    flow = np.zeros((20, 30, 2), F32)
    with pytest.raises(TypeError):
        M.local_correlation(ref, mov)                                  # floor is required
    for bad in (dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor="1"),
                dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=50.0), dict(sigma=43.0, truncate=3.0), dict(truncate=0.0),
                dict(sigma="2"), dict(labels="u8"), dict(labels=1),
                dict(center="mean"), dict(center=1.0), dict(center=(1.0,)), dict(center=(float("nan"), 0.0)),
                dict(lo=0.75), dict(lo=0.9, hi=0.8), dict(lo=-2.0), dict(hi=1.5), dict(min_support=-1.0),
                dict(cell_size=0), dict(cell_size=(3, -1)),
                dict(weight=np.ones((20, 31), F32)), dict(weight=np.ones((20, 30), F64)), dict(weight=np.ones((2, 2), F32)),
                dict(flow=np.zeros((20, 30, 2), F64)), dict(flow=np.zeros((20, 31, 2), F32)), dict(flow=np.zeros((20, 30), F32)),
                dict(flow=[[0.0]]), dict(tmat=np.zeros((3, 3))), dict(tmat=[[1, 0, np.nan], [0, 1, 0]]),
                dict(flow=flow, tmat="identity")):
        with pytest.raises(ValueError):
            M.local_correlation(ref, mov, **dict(dict(floor=1.0), **bad))
    for r_, m_, kw in ((np.zeros((20, 30), F64), mov, {}), (ref, np.zeros((20, 30), np.int32), {}), (ref, np.zeros((20, 30, 3), np.uint8), {}),
                       (ref, np.zeros((19, 30), np.uint8), {}),                       # no flow and unequal shapes
                       (ref, np.zeros((20, 29), np.uint8), {}),
                       (ref, np.zeros((21, 30), np.uint8), dict(flow=flow)),          # a moving image larger than the reference
                       (None, mov, {}), (ref, None, {})):
        with pytest.raises(ValueError):
            M.local_correlation(r_, m_, floor=1.0, **kw)
    with pytest.raises(ValueError):
        M.CorrelationMaps(np.zeros((2, 2), F32), np.zeros((2, 2), F32)).summary()
    maps = M.CorrelationMaps(None, None, agree=np.array([[6, 0]]), disagree=np.array([[1, 3]]), flat=np.array([[1, 0]]),
                             unsupported=np.array([[0, 1]]))
    assert maps.summary() == {"cells": 2, "pixels": 12, "agree": 0.5, "disagree": 4 / 12, "flat": 1 / 12, "unsupported": 1 / 12,
                              "worst_cell": (0, 1), "worst_cell_disagree": 0.75}


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_agree():
    import microaligner_amd
    from microaligner_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_local_correlation"] == sorted(_lib.LOCALCORR_SIGNATURES)
    proto = re.search(r"\bma_local_correlation\s*\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.LOCALCORR_SIGNATURES["ma_local_correlation"][1]) == 21
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES, _lib.FLOWCOMPOSE_SIGNATURES,
              _lib.FLOWINVERT_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.FLOWGRID_SIGNATURES, _lib.FLOWSMOOTH_SIGNATURES,
              _lib.FLOWAFFINE_SIGNATURES, _lib.TEXTURE_SIGNATURES, _lib.DIRECT_SIGNATURES, _lib.FLOWREFINE_SIGNATURES,
              _lib.LANDMARK_SIGNATURES, _lib.TRANSLATION_SIGNATURES, _lib.QUANTILE_SIGNATURES]
    assert not any(set(_lib.LOCALCORR_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_flowsmooth.h"' in open(HEADER).read()
    consts = re.findall(r"#define\s+(MA_[A-Z0-9_]+)\s+(\d+)\b", text)
    assert sorted(n for n, _ in consts) == ["MA_LOCALCORR_CLASSES", "MA_LOCALCORR_MAX_RADIUS"]
    for name, value in consts:
        assert getattr(_lib, name) == int(value), name
    assert _lib.MA_LOCALCORR_MAX_RADIUS == _lib.MA_SMOOTH_MAX_RADIUS       # one check of the taps serves both
    assert _lib.MA_LOCALCORR_CLASSES == R.CLASSES
    assert {"local_correlation", "CorrelationMaps"} <= set(microaligner_amd.__all__)
    assert callable(microaligner_amd.local_correlation) and hasattr(microaligner_amd.device.Context, "local_correlation")


def test_the_source_is_built_and_off_the_measured_path():
    from microaligner_amd import build
    assert build.source_hash() == HASH
    assert "local_correlation.hip" in build.SOURCES and "microaligner_localcorr.h" not in " ".join(build.HEADERS)
    assert [os.path.basename(h) for h in build.SOURCE_HEADERS["local_correlation.hip"]] == \
        ["microaligner_localcorr.h", "microaligner_flowsmooth.h", "cell_grid.h", "window_fir.h", "weight_map.h"]
    users = open(os.path.join(build.CSRC, "window_fir.h")).read().split("#pragma once")[0]
    assert "local_correlation.hip" in users
