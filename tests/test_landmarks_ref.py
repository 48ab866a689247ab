"""Thin-plate splines of landmark pairs (include/microaligner_landmarks.h), the host side: fit_landmarks() against the numpy
statement (tests/_landmarks_ref.py) and scipy's RBFInterpolator, the properties of the model, every refusal before a device
exists, and the wiring of the new source into the build recipe and the bindings."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _landmarks_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402
import microaligner_amd  # noqa: E402
from microaligner_amd import LandmarkFit, _lib, fit_landmarks, landmark_flow, landmark_points  # noqa: E402
from microaligner_amd.device import landmark_flow_params, landmark_points_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_landmarks.h")
SMOOTHINGS = (0.0, 1.0, 100.0, 1e4)
CASES = {"96x161_n40": (96, 161, 40, 1), "37x515_n130": (37, 515, 130, 2)}


def pairs(H, W, n, seed, noise=1.5):
    """n off-grid reference points on an (H, W) frame, one in the central half of a random cell of a lattice (so no two of
    them nearly coincide: the system's condition number stays below the 1.4e6 that the scipy bound below is derived for; 130
    uniformly random points on 37 x 515 come as close as 0.1 px and reach 1e8), and moving points that are a gentle affine map
    of them plus `noise` px of scatter"""
    rng = np.random.default_rng(seed)
    ny = max(1, int(round(np.sqrt(n * H / W))))
    nx = -(-n // ny)
    cy, cx = np.divmod(rng.permutation(ny * nx)[:n], nx)
    r = np.stack([(cx + 0.25 + 0.5 * rng.random(n)) * (W - 1) / nx, (cy + 0.25 + 0.5 * rng.random(n)) * (H - 1) / ny], axis=1)
    m = r @ np.array([[1.01, 0.02], [-0.015, 0.99]]) + [2.5, -1.75] + rng.normal(0, noise, (n, 2))
    return r, m


def spline(f, p):
    """the statement's evaluation of a LandmarkFit at positions p"""
    return R.evaluate(f.cw, f.a6, f.c, f.k, p)


# ---- 1. the fit against the statement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("smoothing", SMOOTHINGS)
def test_fit_matches_the_statement(case, smoothing):
    H, W, n, seed = CASES[case]
    r, m = pairs(H, W, n, seed)
    f, ref = fit_landmarks(r, m, smoothing), R.fit(r, m, smoothing)
    assert isinstance(f, LandmarkFit) and len(f) == n and f.smoothing == smoothing
    assert np.array_equal(f.c, ref["c"]) and f.k == ref["k"] and np.array_equal(f.centres, ref["u"])
    scale = np.abs(ref["w"]).max()
    print("weights: max relative difference", np.abs(f.weights - ref["w"]).max() / scale)
    assert np.abs(f.weights - ref["w"]).max() <= 1e-9 * scale
    assert np.abs(f.affine - ref["a"]).max() <= 1e-9 * np.abs(ref["a"]).max()
    assert f.weights.shape == (n, 2) and f.affine.shape == (2, 3) and f.residual.shape == (n, 2)
    s = ref["K"] @ ref["w"] + np.concatenate([ref["u"], np.ones((n, 1))], axis=1) @ ref["a"].T
    assert np.abs(f.residual - (m - s)).max() <= 1e-9
    energy = float(np.sum(ref["w"] * (ref["K"] @ ref["w"])))
    assert abs(f.bending_energy - energy) <= 1e-9 * max(abs(energy), 1.0)
    # affine_px takes reference pixels to moving pixels: the affine part of s, in pixels
    p = np.array([[0.0, 0.0], [W - 1.0, 0.0], [3.5, H - 1.0]])
    X = (p - f.c) * f.k
    assert np.abs((p @ f.affine_px[:, :2].T + f.affine_px[:, 2]) - (X @ f.affine[:, :2].T + f.affine[:, 2])).max() <= 1e-9
    cw, a6 = R.records(ref)
    assert f.cw.shape == (n, 4) and f.cw.flags.c_contiguous and np.array_equal(f.cw[:, :2], cw[:, :2]) and f.a6.shape == (6,)


# ---- 2. interpolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_the_spline_interpolates_without_smoothing(case):
    H, W, n, seed = CASES[case]
    r, m = pairs(H, W, n, seed)
    f = fit_landmarks(r, m)
    s, _ = spline(f, r)
    print("interpolation: max |s(r_i) - m_i|", np.abs(s - m).max())
    assert np.abs(s - m).max() <= 1e-6
    assert np.abs(f.residual).max() <= 1e-6


# ---- 3. scipy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("smoothing", SMOOTHINGS)
def test_fit_matches_scipys_rbf_interpolator(case, smoothing):
    from scipy.interpolate import RBFInterpolator
    H, W, n, seed = CASES[case]
    r, m = pairs(H, W, n, seed)
    p = np.random.default_rng(seed + 10).random((300, 2)) * [W - 1, H - 1]
    ref = R.fit(r, m, smoothing)
    P = np.concatenate([ref["u"], np.ones((n, 1))], axis=1)
    cond = np.linalg.cond(np.block([[ref["K"] + ref["lam"] * np.eye(n), P], [P.T, np.zeros((3, 3))]]))
    assert cond <= 1.4e6            # what the 1e-8 below is derived for: cond * 2^-53 * |m|, |m| <= 515
    s, _ = spline(fit_landmarks(r, m, smoothing), p)
    want = RBFInterpolator(r, m, kernel="thin_plate_spline", degree=1, smoothing=smoothing)(p)
    print("scipy: condition number", cond, "max difference", np.abs(s - want).max())
    assert np.abs(s - want).max() <= 1e-8


# ---- 4. an exact affine map --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_landmarks_of_an_affine_map_give_the_affine_flow(case):
    H, W, n, seed = CASES[case]
    r, _ = pairs(H, W, n, seed)
    M = np.array([[1.02, -0.03, 4.25], [0.025, 0.97, -2.5]])
    m = r @ M[:, :2].T + M[:, 2]
    f = fit_landmarks(r, m)
    print("affine: max |w|", np.abs(f.weights).max())
    assert np.abs(f.weights).max() <= 1e-9
    assert np.abs(f.affine_px - M).max() <= 1e-9
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    p = np.stack([gx.ravel(), gy.ravel()], axis=1)[::7]
    s, _ = spline(f, p)
    want = p - (p @ M[:, :2].T + M[:, 2])          # the affine flow p - M p
    assert np.abs((p - s) - want).max() <= 1e-9


# ---- 5. smoothing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_smoothing_trades_residual_for_bending(case):
    H, W, n, seed = CASES[case]
    r, m = pairs(H, W, n, seed)
    fits = [fit_landmarks(r, m, sm) for sm in SMOOTHINGS]
    rms = [float(np.sqrt(np.mean(np.sum(f.residual ** 2, axis=1)))) for f in fits]
    energy = [f.bending_energy for f in fits]
    print("residual rms", rms, "bending energy", energy)
    assert all(b >= a for a, b in zip(rms, rms[1:])) and rms[0] <= 1e-6 < rms[1]
    assert all(b <= a for a, b in zip(energy, energy[1:])) and energy[-1] >= 0


# ---- 6. permutation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("smoothing", (0.0, 100.0))
def test_the_spline_does_not_depend_on_the_order_of_the_landmarks(case, smoothing):
    """Within the evaluation bound (n + 8) * 2^-53 * mag of the header's float64 chain, per position and component: the
    records of one fit in another order (the statement sums without rounding, so the order cannot show), and a fit of the
    permuted pairs, which solves a differently pivoted system."""
    H, W, n, seed = CASES[case]
    r, m = pairs(H, W, n, seed)
    perm = np.random.default_rng(seed + 20).permutation(n)
    p = np.random.default_rng(seed + 21).random((300, 2)) * [W - 1, H - 1]
    f = fit_landmarks(r, m, smoothing)
    s, mag = spline(f, p)
    s_rec, _ = R.evaluate(f.cw[perm], f.a6, f.c, f.k, p)
    assert np.all(np.abs(s_rec - s) <= R.bound(mag, n))
    g = fit_landmarks(r[perm], m[perm], smoothing)
    s_fit, _ = spline(g, p)
    print("permuted fit: max difference", np.abs(s_fit - s).max(), "evaluation bound", R.bound(mag, n).max())
    print("permuted fit: worst ratio to the bound", (np.abs(s_fit - s) / R.bound(mag, n)).max())
    assert np.all(np.abs(s_fit - s) <= R.bound(mag, n))
    assert np.abs(g.weights - f.weights[perm]).max() <= 1e-9 * np.abs(f.weights).max()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import microaligner_amd.device as dev
    import microaligner_amd.optflow_reg.landmarks as mod

    def refuse(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(mod, "get_context", refuse)
    monkeypatch.setattr(dev, "get_context", refuse)


def _good(n=7, seed=3):
    return pairs(96, 161, n, seed)


def _bad_pairs():
    r, m = _good()
    line = np.stack([np.arange(7.0) * 3, np.arange(7.0) * 1.5 + 2], axis=1)
    nan, inf = r.copy(), m.copy()
    nan[2, 1], inf[4, 0] = np.nan, np.inf
    big = pairs(96, 161, 4097, 4)
    dup = r.copy()
    dup[5] = dup[1]
    near = r.copy()
    near[5] = near[1] + [1e-7, 0.0]
    return {"not_n_by_2": (r.T, m.T), "three_columns": (np.zeros((7, 3)), np.zeros((7, 3))), "unequal": (r, m[:6]),
            "one_dimensional": (r.ravel(), m.ravel()), "text": ("ab", "cd"), "nan_reference": (nan, m), "inf_moving": (r, inf),
            "two_pairs": (r[:2], m[:2]), "none": (r[:0], m[:0]), "too_many": big, "collinear": (line, m),
            "all_equal": (np.tile(r[:1], (7, 1)), m), "duplicate": (dup, m), "near_duplicate": (near, m)}


@pytest.mark.parametrize("what", list(_bad_pairs()))
def test_bad_landmarks_raise_before_device_work(no_device, what):
    r, m = _bad_pairs()[what]
    with pytest.raises(ValueError):
        fit_landmarks(r, m)
    with pytest.raises(ValueError):
        landmark_flow((r, m), (96, 161))
    with pytest.raises(ValueError):
        landmark_points((r, m), np.zeros((3, 2)))


@pytest.mark.parametrize("smoothing", [-1.0, -1e-300, float("nan"), float("inf"), "1", None, True])
def test_bad_smoothing_raises_before_device_work(no_device, smoothing):
    r, m = _good()
    with pytest.raises(ValueError):
        fit_landmarks(r, m, smoothing)


def test_the_self_check_catches_a_near_duplicate_and_smoothing_accepts_it(no_device):
    r, m = _good()
    r[5] = r[1] + [1e-7, 0.0]                       # not exactly equal: only the self-check can see it
    with pytest.raises(ValueError, match="misses its own equations"):
        fit_landmarks(r, m)
    f = fit_landmarks(r, m, smoothing=1.0)
    assert np.all(np.isfinite(f.weights)) and np.abs(f.residual - f.smoothing * f.k ** 2 * f.weights).max() <= 1e-6
    r[5] = r[1]                                     # exactly equal: refused without smoothing, accepted with it
    with pytest.raises(ValueError, match="equal"):
        fit_landmarks(r, m)
    assert len(fit_landmarks(r, m, smoothing=1.0)) == 7


def test_bad_evaluation_arguments_raise_before_device_work(no_device):
    f = fit_landmarks(*_good())
    for shape in ((0, 5), (5, 0), (5,), (5, 6, 2), ((1 << 24) + 1, 4), (4, (1 << 24) + 1), (4.0, 5), None, "ab"):
        with pytest.raises(ValueError):
            landmark_flow(f, shape)
    for stride in (0, -1, 1.5, True, "2", 1 << 31):
        with pytest.raises(ValueError):
            landmark_flow(f, (9, 8), stride=stride)
    with pytest.raises(ValueError):
        landmark_flow(f, (9, 8), smoothing=1.0)     # smoothing belongs to the fit
    with pytest.raises(ValueError):
        landmark_flow("fit", (9, 8))
    for pts in (np.zeros((3, 2), np.float32), np.zeros((3, 3)), np.zeros(6), [[1.0, 2.0]], None):
        with pytest.raises(ValueError):
            landmark_points(f, pts)
    ok = dict(cw=f.cw, a6=f.a6, c=f.c, k=f.k)
    assert landmark_flow_params(**ok, shape=(9, 8), stride=3)[5:] == (9, 8, 3)
    assert landmark_points_params(**ok, points=np.zeros((0, 2)))[5].shape == (0, 2)
    assert landmark_flow_params(np.zeros((0, 4)), f.a6, f.c, f.k, (1, 1))[0].shape == (0, 4)     # n = 0: the affine part alone
    nan_cw = f.cw
    nan_cw[3, 2] = np.nan
    for bad in (dict(cw=f.cw.astype(np.float32)), dict(cw=f.cw[:, :3]), dict(cw=f.cw.ravel()), dict(cw=nan_cw),
                dict(cw=np.zeros((_lib.MA_LANDMARK_MAX + 1, 4))), dict(a6=f.a6[:5]), dict(a6=np.full(6, np.inf)),
                dict(a6="abcdef"), dict(c=[np.nan, 0.0]), dict(c=[1.0]), dict(k=float("inf")), dict(k=None)):
        with pytest.raises(ValueError):
            landmark_flow_params(**dict(ok, **bad), shape=(9, 8))
        with pytest.raises(ValueError):
            landmark_points_params(**dict(ok, **bad), points=np.zeros((2, 2)))


# ---- 8. wiring --------------------------------------------------------------------------------------------------------------------
def test_header_library_bindings_and_build_recipe_agree():
    from microaligner_amd import build
    build.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_landmark_flow", "ma_landmark_points"] == sorted(_lib.LANDMARK_SIGNATURES)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_landmarks.h but not exported"
        proto = re.search(r"\b" + n + r"\s*\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.LANDMARK_SIGNATURES[n][1]), n
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES, _lib.FLOWCOMPOSE_SIGNATURES,
              _lib.FLOWINVERT_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.FLOWGRID_SIGNATURES, _lib.FLOWSMOOTH_SIGNATURES,
              _lib.FLOWAFFINE_SIGNATURES, _lib.TEXTURE_SIGNATURES, _lib.DIRECT_SIGNATURES, _lib.FLOWREFINE_SIGNATURES]
    assert not any(set(_lib.LANDMARK_SIGNATURES) & set(t) for t in others)
    consts = dict(re.findall(r"#define\s+(MA_[A-Z0-9_]+)\s+(\d+)\b", text))
    assert sorted(consts) == ["MA_LANDMARK_CHUNK", "MA_LANDMARK_MAX"]
    for name, value in consts.items():
        assert getattr(_lib, name) == int(value), name
    assert _lib.MA_LANDMARK_CHUNK >= 1 and _lib.MA_LANDMARK_MAX == 1 << 20
    assert {"LandmarkFit", "fit_landmarks", "landmark_flow", "landmark_points"} <= set(microaligner_amd.__all__)
    import microaligner_amd.optflow_reg as opt
    assert all(getattr(opt, n) is getattr(microaligner_amd, n)
               for n in ("LandmarkFit", "fit_landmarks", "landmark_flow", "landmark_points"))
    # the C entries refuse a NULL ctx before they touch a device
    a6 = (_lib.C.c_double * 6)(1, 0, 0, 0, 1, 0)
    assert lib.ma_landmark_flow(None, None, 0, a6, 0.0, 0.0, 1.0, 4, 4, 1, None) == _lib.MA_EINVAL
    assert lib.ma_landmark_points(None, None, 0, a6, 0.0, 0.0, 1.0, None, 0, None) == _lib.MA_EINVAL
    assert b"invalid argument" in lib.ma_last_error()


def test_the_new_source_stays_out_of_the_measured_path_hash():
    from microaligner_amd import build
    assert build.source_hash() == HASH == _lib.source_hash()
    assert "landmarks.hip" in build.SOURCES
    assert [os.path.abspath(h) for h in build.SOURCE_HEADERS["landmarks.hip"]] == [HEADER]
    assert HEADER not in [os.path.abspath(h) for h in build.HEADERS]
