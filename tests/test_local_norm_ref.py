"""The local contrast normalisation without a GPU (include/microaligner_localnorm.h): the numpy float32 statement
(tests/_local_norm_ref.py) against its float64 twin, the invariance to a gain and an offset that is the point of it, what it
does for Farneback on a pair under a gain field, the header against the library and the bindings, and every argument that
is refused without a device."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_smooth_ref as S  # noqa: E402
import _local_norm_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402

pytest.register_assert_rewrite("_gpu_cases")
import _gpu_cases as G  # noqa: E402  (the registry: CASES, EXEMPT, declared_entries)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_localnorm.h")
F32, F64 = np.float32, np.float64
K_MEASURED = 1.58          # the largest K of the three cases below (0.78, 0.49, 1.58)
K_ALLOWED = 4 * K_MEASURED


def taps_of(r):
    sigma = r / 3.0
    taps = S.gaussian_taps(sigma, (r - 0.5) / sigma)         # ceil(r - 0.5) = r whatever the rounding of the product
    assert len(taps) == r + 1
    return taps


def same_bits(got, exp):
    assert got.dtype == exp.dtype and got.shape == exp.shape
    if got.dtype != F32:
        return np.array_equal(got, exp)
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(got.view(np.uint32)[~gn], exp.view(np.uint32)[~en])


def twin_cases():
    """(name, image, taps, floor, weight): the three cases of the comparison"""
    w, _ = R.make_weight(37, 515)
    mask = np.ones((257, 300), np.uint8)
    mask[100:140, 50:120] = 0
    return [("96 x 160 uint8", R.make_image(96, 160, np.uint8), taps_of(7), R.floor_of(np.uint8), None),
            ("37 x 515 uint16, float weight", R.make_image(37, 515, np.uint16), taps_of(12), R.floor_of(np.uint16), w),
            ("257 x 300 float32, mask with a hole", R.make_image(257, 300, np.float32), taps_of(21), R.floor_of(np.float32), mask)]


def test_float32_statement_against_the_float64_twin():
    """|z32 - z64| <= K 2^-24 (max|x| / sqrt(floor) + |z64|) with K = 4 x 1.58 = 6.32, floor = (0.01 of the dtype's range)^2.
    The first term is the cancellation in d = x - mu: mu carries an error of a few ulp of max|x|, and z is d over at least
    sqrt(floor).  Measured K: 0.78 (96 x 160 uint8, r = 7), 0.49 (37 x 515 uint16 with the float weight, r = 12), 1.58
    (257 x 300 float32 with the mask, r = 21).  The uint8 outputs may differ from the twin's by at most one level; the share
    that differs is reported, not capped: none of the pixels in any of the three cases."""
    worst = 0.0
    for name, img, taps, floor, weight in twin_cases():
        a = R.normalize_local_ref(img, taps, floor, 4.0, weight, 0.05)
        b = R.normalize_local_f64(img, taps, floor, 4.0, weight, 0.05)
        has = ~np.isnan(b["z"])
        assert np.array_equal(has, ~np.isnan(a["z"])) and has.sum() > 0.5 * img.size
        xmax = np.abs(np.asarray(img, F64)[a["live"]]).max()
        bound = 2.0 ** -24 * (xmax / np.sqrt(F64(F32(floor))) + np.abs(b["z"][has]))
        k = (np.abs(a["z"][has].astype(F64) - b["z"][has]) / bound).max()
        step = np.abs(a["u8"].astype(np.int16) - b["u8"].astype(np.int16))
        print(f"{name}: K = {k:.2f}; u8 differs at {100.0 * (step > 0).mean():.3f} % of the pixels, by at most {step.max()}")
        assert step.max() <= 1
        assert (a["u8"][~has] == 128).all() and not a["f32"][~has].any()
        worst = max(worst, k)
    assert worst <= K_ALLOWED, worst
    assert worst >= K_MEASURED / 4, f"K_MEASURED is stale: measured {worst:.2f}"


@pytest.mark.parametrize("g, b", [(2.5, 37.0), (0.3, -11.0)])
def test_a_gain_and_an_offset_leave_the_float64_twin_unchanged(g, b):
    for name, img, taps, floor, weight in twin_cases():
        x = np.asarray(img, F64)
        z0 = R.normalize_local_f64(x, taps, floor, np.inf, weight, 0.05)["z"]
        z1 = R.normalize_local_f64(g * x + b, taps, floor * g * g, np.inf, weight, 0.05)["z"]
        has = ~np.isnan(z0)
        assert np.array_equal(has, ~np.isnan(z1)) and np.abs(z1[has] - z0[has]).max() <= 1e-9, name


def test_a_power_of_two_gain_leaves_the_float32_statement_bit_for_bit():
    _, img, taps, floor, weight = twin_cases()[2]
    a = R.normalize_local_ref(img, taps, floor, 4.0, weight, 0.05)
    b = R.normalize_local_ref(img * F32(4), taps, floor * 16, 4.0, weight, 0.05)
    assert same_bits(a["f32"], b["f32"]) and same_bits(a["u8"], b["u8"]) and a["counts"] == b["counts"]
    assert a["counts"][R.FLAT] > 0 and a["counts"][R.DROPPED] == 40 * 70 and np.ptp(a["u8"]) > 200


def test_counts_and_the_no_contrast_value():
    """dropped + unsupported + the pixels with a z are every pixel; flat windows come out near 128; a masked pixel and a
    pixel without support come out as exactly 128 / +0.0"""
    img = R.make_image(64, 96, np.uint16)
    w, _ = R.make_weight(64, 96)
    r = R.normalize_local_ref(img, taps_of(3), R.floor_of(np.uint16), 2.0, w, 0.5)
    dropped, unsupported, flat, clipped = r["counts"]
    has = ~np.isnan(r["z"])
    assert dropped + unsupported + has.sum() == img.size and dropped > 0 and unsupported > 0 and flat > 0 and clipped > 0
    assert (r["u8"][~has] == 128).all() and not r["f32"][~has].any() and not np.signbit(r["f32"][~has]).any()
    assert np.abs(r["f32"]).max() == 2.0 and r["u8"].max() == 255
    # the uint8 output is not clipped at -clip: z = -clip is level 1, and level 0 is everything below -clip * 128 / 127
    assert r["u8"].min() == 0 and (r["u8"][r["f32"] == -2.0] <= 1).all() and (r["u8"][r["f32"] == 2.0] == 255).all()
    assert r["u8"].dtype == np.uint8 and r["f32"].dtype == F32
    assert R.normalize_local_ref(img, taps_of(3), 1.0, np.inf)["u8"] is None


# ---- what it is for ----------------------------------------------------------------------------------------------------------
def usefulness_rows():
    """endpoint error (median, p99, max in px, 64 px border left out) of the oracle's Farneback, 3 iterations, on
    synthetic.make_pair(512, 512, seed=1) at windows 31 and 99: the pair as it is and under a gain field, as it is, min/max
    to u8, and through the statement (clip 4, u8 output, floor 1)"""
    from microaligner_amd import synthetic
    from oracle import oracle as O
    O.build()
    H = W = 512
    ref, mov = synthetic.make_pair(H, W, seed=1)
    g, o = R.gain_field(H, W)
    gained = (mov * g + o + 40).astype(F32)
    dx, dy = synthetic.displacement(H, W)
    truth = np.stack([dx + 0 * dy, dy + 0 * dx], -1)

    def norm(img, sigma):
        return R.normalize_local_ref(img, S.gaussian_taps(sigma), 1.0, 4.0)["u8"]

    def epe(a, b, win):
        e = np.sqrt(((O.calc_optical_flow_farneback(b, a, win, 3) - truth) ** 2).sum(-1))[64:-64, 64:-64]
        return float(np.median(e)), float(np.percentile(e, 99)), float(e.max())
    pairs = [("clean", ref, mov), ("gain field, f32 as is", ref, gained),
             ("gain field, each image min/max to u8", O.normalize_minmax_u8(ref), O.normalize_minmax_u8(gained)),
             ("gain field, both normalised, sigma 8", norm(ref, 8), norm(gained, 8)),
             ("gain field, both normalised, sigma 16", norm(ref, 16), norm(gained, 16)),
             ("clean, both normalised, sigma 16", norm(ref, 16), norm(mov, 16))]
    return {name: {win: epe(a, b, win) for win in (31, 99)} for name, a, b in pairs}


def test_normalised_inputs_give_farneback_its_accuracy_back_under_a_gain_field():
    """Measured (median / p99 / max, px):           window 31               window 99
         clean                                    0.105 / 0.311 / 0.445   0.254 / 0.476 / 0.537
         gain field, f32 as is                    0.186 / 0.685 / 1.161   0.254 / 0.527 / 0.636
         gain field, each image min/max to u8     0.272 / 1.140 / 2.166   0.261 / 0.600 / 0.734
         gain field, both normalised, sigma 8     0.101 / 0.295 / 0.463   0.238 / 0.448 / 0.537
         gain field, both normalised, sigma 16    0.104 / 0.300 / 0.469   0.250 / 0.480 / 0.556
         clean, both normalised, sigma 16         0.101 / 0.299 / 0.446   0.250 / 0.477 / 0.541
    Asserted: only the order at window 31, p99 of the normalised gain pair < p99 of the gain pair as it is."""
    rows = usefulness_rows()
    for name, by_win in rows.items():
        print(f"{name:40s}", "   ".join(" / ".join(f"{v:.3f}" for v in by_win[win]) for win in (31, 99)))
    for sigma in (8, 16):
        assert rows[f"gain field, both normalised, sigma {sigma}"][31][1] < rows["gain field, f32 as is"][31][1]


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree():
    import microaligner_amd
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_normalize_local"] == sorted(_lib.LOCALNORM_SIGNATURES)
    assert hasattr(lib, "ma_normalize_local"), "declared in microaligner_localnorm.h but not exported"
    proto = re.search(r"\bma_normalize_local\s*\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.LOCALNORM_SIGNATURES["ma_normalize_local"][1]) == 15
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES") and t != "LOCALNORM_SIGNATURES"]
    assert len(others) >= 20 and not any(set(_lib.LOCALNORM_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_flowsmooth.h"' in open(HEADER).read()
    assert 'alignment rule of microaligner_hip.h ("Device pointers")' in open(HEADER).read()
    consts = re.findall(r"#define\s+(MA_[A-Z0-9_]+)\s+(\d+)\b", text)
    assert sorted(n for n, _ in consts) == ["MA_LOCALNORM_COUNTS", "MA_LOCALNORM_MAX_RADIUS"]
    for name, value in consts:
        assert getattr(_lib, name) == int(value), name
    assert _lib.MA_LOCALNORM_MAX_RADIUS == _lib.MA_SMOOTH_MAX_RADIUS       # one check of the taps serves both
    assert _lib.MA_LOCALNORM_COUNTS == R.COUNTS == len(microaligner_amd.LocalNormInfo._fields)
    assert {"normalize_local", "LocalNormInfo"} <= set(microaligner_amd.__all__)
    assert callable(microaligner_amd.normalize_local) and hasattr(microaligner_amd.device.Context, "normalize_local")
    assert microaligner_amd.LocalNormInfo._fields == ("dropped", "unsupported", "flat", "clipped")


def test_the_source_is_built_and_off_the_measured_path():
    from microaligner_amd import build
    assert build.source_hash() == HASH
    assert "local_norm.hip" in build.SOURCES and "microaligner_localnorm.h" not in " ".join(build.HEADERS)
    assert [os.path.basename(h) for h in build.SOURCE_HEADERS["local_norm.hip"]] == \
        ["microaligner_localnorm.h", "microaligner_flowsmooth.h", "window_fir.h", "weight_map.h", "call_counts.h"]
    for shared in ("window_fir.h", "weight_map.h", "call_counts.h"):
        assert "local_norm.hip" in open(os.path.join(build.CSRC, shared)).read().split("#pragma once")[0], shared
    src = open(os.path.join(build.CSRC, "local_norm.hip")).read()
    for word in ("wf_row_plane", "wf_acquire", "wf_finish", "wf_taps", "d_weight_px", "ma_weight_check", "d_wave_tally"):
        assert word in src, word


def test_the_cases_are_in_the_registry():
    """the GPU cases that run ma_normalize_local on stale scratch memory and at shifted addresses (tests/_gpu_cases)"""
    cases = [c for c in G.CASES if c.entries == ("ma_normalize_local",)]
    assert len(cases) == 2 and "ma_normalize_local" in G.declared_entries() and "ma_normalize_local" not in G.EXEMPT


# ---- refused arguments -----------------------------------------------------------------------------------------------------
H, W = 6, 10
IMG = np.zeros((H, W), np.uint16)


def test_local_norm_params_without_a_device():
    from microaligner_amd import _lib as L
    from microaligner_amd import device as D
    taps = D.gaussian_taps(1.0)
    got = D.local_norm_params(IMG, taps, 2.5)
    assert got == (H, W, L.MA_U16, got[3], 3, 2.5, 4.0, L.MA_SMOOTH_WEIGHT_NONE, 0.0, ("u8",)) and got[3].dtype == F32
    got = D.local_norm_params(IMG.astype(F32), taps, 1, np.inf, np.ones((H, W), np.uint8), 0.5, ["f32"])
    assert got[2] == L.MA_F32 and got[5:] == (1.0, np.inf, L.MA_SMOOTH_WEIGHT_U8, 0.5, ("f32",))
    assert D.local_norm_params(IMG, taps, 1, 2, np.ones((H, W), F32), want=("f32", "u8"))[7:] == (L.MA_SMOOTH_WEIGHT_F32, 0.0, ("f32", "u8"))
    nan, inf = float("nan"), float("inf")
    bad = [dict(img=IMG.astype(np.int32)), dict(img=IMG.astype(F64)), dict(img=IMG[0]), dict(img=IMG[None]), dict(img=[[1, 2]]),
           dict(img=np.zeros((0, 4), np.uint8)), dict(img=np.zeros((4, 0), np.uint8)),
           dict(taps=taps.astype(F64)), dict(taps=list(taps)), dict(taps=taps[:1]), dict(taps=np.zeros(130, F32) + F32(0.1)),
           dict(taps=np.array([0, 0.5], F32)), dict(taps=np.array([0.5, -0.1], F32)), dict(taps=np.array([0.5, nan], F32)),
           dict(taps=np.array([0.5, inf], F32)), dict(taps=taps[None]),
           dict(floor=0), dict(floor=-1.0), dict(floor=nan), dict(floor=inf), dict(floor=1e-50), dict(floor=1e39), dict(floor="1"),
           dict(floor=None), dict(floor=True),
           dict(clip=0), dict(clip=-4.0), dict(clip=nan), dict(clip=1e-50), dict(clip=inf), dict(clip="4"), dict(clip=None),
           dict(clip=1e39), dict(clip=inf, want=("f32", "u8")),
           dict(min_support=-0.1), dict(min_support=nan), dict(min_support=inf), dict(min_support="0"),
           dict(weight=np.ones((H, W), F64)), dict(weight=np.ones((W, H), F32)), dict(weight=np.ones((2, 3), F32)),
           dict(weight=[[1.0] * W] * H), dict(weight=np.ones((H, W, 1), np.uint8)),
           dict(want=()), dict(want="u8"), dict(want=("u8", "u8")), dict(want=("u16",)), dict(want=("f32", 1)), dict(want=None)]
    ok = dict(img=IMG, taps=taps, floor=1.0)
    for kw in bad:
        with pytest.raises(ValueError):
            D.local_norm_params(**dict(ok, **kw))
    D.local_norm_params(**dict(ok, clip=inf, want=("f32",)))
    D.local_norm_params(**dict(ok, clip=1e39, want=("f32",)))            # +Inf as float32


def test_normalize_local_refuses_without_a_device(monkeypatch):
    import microaligner_amd as M
    from microaligner_amd import device as D

    def no_context(*a, **k):
        raise AssertionError("a refused call must not reach the device")
    monkeypatch.setattr(D, "get_context", no_context)
    nan, inf = float("nan"), float("inf")
    bad = [dict(sigma=0), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(sigma="4"), dict(sigma=50.0),
           dict(truncate=0), dict(truncate=nan), dict(sigma=16.0, truncate=9.0),
           dict(dtype="uint16"), dict(dtype="u8"), dict(dtype=None), dict(dtype=np.uint16), dict(dtype=8),
           dict(on_device=1), dict(on_device=None), dict(return_info="yes"), dict(return_info=0),
           dict(floor=0), dict(floor=nan), dict(floor=-1), dict(floor=inf), dict(clip=0), dict(clip=nan), dict(clip=-1),
           dict(clip=inf), dict(clip=inf, dtype="uint8"),
           dict(min_support=-1), dict(min_support=nan), dict(weight=np.ones((W, H), F32)), dict(weight=np.ones((H, W), F64)),
           dict(weight=np.ones((2, 3), F32)), dict(img=IMG.astype(np.int16)), dict(img=IMG[0]), dict(img=np.zeros((0, 3), F32)),
           dict(img=[[1.0, 2.0]])]
    ok = dict(img=IMG, sigma=2.0, floor=1.0)
    for kw in bad:
        with pytest.raises(ValueError):
            args = dict(ok, **kw)
            M.normalize_local(args.pop("img"), **args)
    with pytest.raises(TypeError):
        M.normalize_local(IMG, 2.0)                       # floor has no default: it is on the data's scale
    with pytest.raises(TypeError):
        M.normalize_local(IMG, 2.0, 1.0)                  # and is given by name
    with pytest.raises(AssertionError):
        M.normalize_local(IMG, 2.0, floor=1.0, clip=inf, dtype="float32")     # a valid call goes on to the device
    with pytest.raises(AssertionError):
        M.normalize_local(IMG, 2.0, floor=1.0, dtype=np.float32)
