"""The host half of the affine split of a flow (microaligner_amd/optflow_reg/flow_affine.py) against the numpy statement of
include/microaligner_flowaffine.h (tests/_flow_affine_ref.py), without a device: the solve from the 14 sums against a fit
that does not use them, join(split(F)), the least-squares property, the rank rule, the trim rounds, the per-cell maps, the
argument checks and the plumbing of the new source."""
import math
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_affine_ref as R  # noqa: E402
from microaligner_amd import FlowAffineMaps, _lib, build, fit_flow_affine, join_flow, local_affine, split_flow  # noqa: E402
from microaligner_amd.optflow_reg import flow_affine as FA  # noqa: E402

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 16 x the largest deviation of the solve from the independent fit seen over CASES x MODELS (2.3e-13, see
# test_the_solve_from_moments_is_the_independent_fit), floor 1e-13
SOLVE_TOL = 16 * 2.3e-13


def cases():
    return [("bumpy", R.bumpy_flow(), None),
            ("dyadic affine 37 x 515", R.affine_flow((37, 515), R.DYADIC_AFFINE), R.DYADIC_AFFINE),
            ("dyadic affine 96 x 161", R.affine_flow((96, 161), R.DYADIC_AFFINE), R.DYADIC_AFFINE),
            ("dyadic similarity 96 x 161", R.affine_flow((96, 161), R.DYADIC_SIMILARITY), R.DYADIC_SIMILARITY)]


@pytest.fixture(scope="module")
def case_moments():
    return [(name, f, inv, R.moments_ref(f)[0][0, 0]) for name, f, inv in cases()]


def solve_abs(sums, shape, model):
    T, deficient = FA.solve_flow_affine(sums, model)
    return FA._to_absolute(T, shape), bool(deficient)


def test_the_solve_from_moments_is_the_independent_fit(case_moments):
    """All four models on the bumpy flow, two exactly affine flows (dyadic inverse matrix, so the flow is exact in
    float32) and a dyadic similarity: the package's solve, fed the statement's fsum moments, against lstsq over the
    pixels / the direct minimisation.  Measured: largest deviation 2.3e-13 ("similarity" on the 37 x 515 strip, in the
    translation, where lstsq's own error in absolute coordinates dominates); the exactly affine flows return the
    inverse of their matrix to 1.8e-14 (37 x 515) and 1.1e-14 (96 x 161), the similarity to 7.5e-15 under both
    "affine" and "similarity"."""
    worst = 0.0
    for name, f, inv, sums in case_moments:
        for model in R.MODELS:
            got, deficient = solve_abs(sums, f.shape, model)
            assert not deficient
            dev = float(np.abs(got - R.fit_ref(f, model)).max())
            print(f"{name:28s} {model:12s} deviation from the independent fit {dev:.3g}")
            worst = max(worst, dev)
            assert dev <= SOLVE_TOL, (name, model, dev)
        if inv is not None:
            for model in ("affine", "similarity") if "similarity" in name else ("affine",):
                dev = float(np.abs(solve_abs(sums, f.shape, model)[0] - R.inverse(inv)).max())
                print(f"{name:28s} {model:12s} deviation from the exact matrix {dev:.3g}")
                assert dev <= SOLVE_TOL
    print(f"largest deviation {worst:.3g}")
    assert SOLVE_TOL >= 1e-13


def test_the_order_of_summation_moves_the_fit_by_less_than_the_gpu_factor():
    """The GPU sums in another order than fsum; its end-to-end tolerance is 4 x SOLVE_TOL.  The spread of the solved
    matrix between fsum, numpy.sum (pairwise) and a sequential sum of the same terms, measured over the cases: 1.6e-13 on
    the bumpy flow (the sequential sum) and 0 on the exactly affine ones, whose terms add without rounding: inside
    SOLVE_TOL (3.7e-12) itself, so the factor 4 leaves room for any order."""
    worst = 0.0
    for name, f, _ in cases():
        terms = R.pixel_terms(f)[0].reshape(-1, 14)
        variants = [np.array([math.fsum(terms[:, k]) for k in range(14)]), terms.sum(0), np.cumsum(terms, 0)[-1]]
        for model in R.MODELS:
            mats = [solve_abs(s, f.shape, model)[0] for s in variants]
            spread = max(float(np.abs(m - mats[0]).max()) for m in mats[1:])
            print(f"{name:28s} {model:12s} spread over the orders of summation {spread:.3g}")
            worst = max(worst, spread)
    print(f"largest spread {worst:.3g}")
    assert worst <= SOLVE_TOL


def split_join(f, model):
    sums = R.moments_ref(f)[0][0, 0]
    T = solve_abs(sums, f.shape, model)[0]
    rest = R.apply_ref(f, T)
    return T, rest, R.apply_ref(rest, R.inverse(T))


@pytest.mark.parametrize("model", R.MODELS)
def test_join_of_split_is_the_flow(model):
    """join(split(F)) = F within 2^-23 max(1, max|F|): one float32 rounding of the residual and one of the result"""
    for name, f, _ in cases():
        T, rest, back = split_join(f, model)
        err = float(np.abs(back.astype(F64) - f.astype(F64)).max())
        bound = 2.0 ** -23 * max(1.0, float(np.abs(f).max()))
        print(f"{name:28s} {model:12s} join(split) error {err:.3g} (bound {bound:.3g})")
        assert err <= bound


@pytest.mark.parametrize("model", R.MODELS)
def test_the_residual_is_the_smallest_of_its_model(model):
    """The RMS of the residual is at or below the flow's (the identity belongs to every model), equals the RMS the sums
    predict, and does not fall when the matrix is perturbed within its model"""
    f = R.bumpy_flow()
    sums = R.moments_ref(f)[0][0, 0]
    Tc = FA.solve_flow_affine(sums, model)[0]
    T = FA._to_absolute(Tc, f.shape)
    rms_flow, rms_rest = R.weighted_rms(f), R.weighted_rms(f, T)
    print(f"{model}: flow RMS {rms_flow:.4g} px, residual RMS {rms_rest:.4g} px")
    assert abs(float(FA._rms(sums)) - rms_flow) <= 1e-12 * rms_flow
    assert rms_rest <= rms_flow
    if model == "affine":
        assert rms_rest < 0.35          # the smooth field has 0.3 px RMS, the similarity 4 px
    rng = np.random.default_rng(3)
    for _ in range(40):
        P = Tc.copy()
        k = rng.uniform(-1, 1, 6) * np.array([1e-4, 1e-4, 1e-2, 1e-4, 1e-4, 1e-2])
        if model == "affine":
            P += k.reshape(2, 3)
        else:
            P[:, 2] += k[[2, 5]]
            if model != "translation":
                ang = math.atan2(Tc[1, 0], Tc[0, 0]) + k[0]
                sc = math.hypot(Tc[0, 0], Tc[1, 0]) * (1 + (k[1] if model == "similarity" else 0.0))
                P[:, :2] = sc * np.array([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]])
        assert R.weighted_rms(f, FA._to_absolute(P, f.shape)) >= rms_rest * (1 - 1e-12)


def rotation_flow(shape, deg=2.0):
    H, W = shape
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    th = math.radians(deg)
    return np.stack([x - (math.cos(th) * x - math.sin(th) * y + 0.5), y - (math.sin(th) * x + math.cos(th) * y - 0.25)],
                    -1).astype(F32)


@pytest.mark.parametrize("shape, deficient", [
    ((1, 64), {"affine": True, "similarity": False, "rigid": False, "translation": False}),
    ((64, 1), {"affine": True, "similarity": False, "rigid": False, "translation": False}),
    ((1, 1), {"affine": True, "similarity": True, "rigid": True, "translation": False}),
    ((2, 3), {"affine": False, "similarity": False, "rigid": False, "translation": False})])
def test_the_rank_rule(shape, deficient):
    """a strip's sampling positions lie on a line: no affine fit, but a similarity; one pixel fixes a translation only"""
    f = rotation_flow(shape)
    sums = R.moments_ref(f)[0][0, 0]
    for model in R.MODELS:
        T, d = FA.solve_flow_affine(sums, model)
        assert bool(d) == deficient[model], (shape, model)
        assert np.isnan(T).all() if deficient[model] else np.isfinite(T).all()
        if not deficient[model] and shape != (1, 1):
            assert np.abs(FA._to_absolute(T, shape) - R.fit_ref(f, model)).max() <= 1e-9
        if deficient[model]:
            with pytest.raises(ValueError, match="rank deficient"):
                FA.fit_from_moments(lambda prior, clip: (sums, (1, 0, 0, 0)), model)
    # no weighted pixel at all: deficient for every model
    zero = R.moments_ref(f, np.zeros(shape, np.uint8))[0][0, 0]
    assert all(bool(FA.solve_flow_affine(zero, m)[1]) for m in R.MODELS)


def test_the_trim_rounds_take_a_corrupted_block_out():
    """A 30 x 50 block of the bumpy flow moved by 25 px drags the untrimmed fit by pixels.  With trim = 2 px (the smooth
    field stays below 0.85 px, the block is 25 px off) the rounds end with exactly the block trimmed, stop when the counts
    repeat, and the matrix is the independent fit over the pixels outside the block.  Measured, as the largest
    displacement of an image corner against the uncorrupted fit: 9.2 px untrimmed, 0.33 px after one round (which trims
    10022 pixels, most of them good), 0.049 px from the second on (the fit without the block's pixels, whose share of the
    smooth field is then missing); the third round repeats the second's counts and ends the loop."""
    clean = R.bumpy_flow()
    f = clean.copy()
    block = (slice(20, 50), slice(40, 90))
    f[block] += F32(25.0)
    keep = np.ones(f.shape[:2], np.uint8)
    keep[block] = 0
    H, W = f.shape[:2]
    corners = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], F64)
    T0 = R.fit_ref(clean)

    def corner_error(Tc):
        return float(np.abs(corners @ (FA._to_absolute(Tc, f.shape) - T0).T).max())

    calls = []

    def moments(prior, clip):
        sums, counts, _ = R.moments_ref(f, None, None, prior, clip)
        calls.append(corner_error(FA.solve_flow_affine(sums[0, 0])[0]))
        return sums[0, 0], counts[0, 0]

    Tc, per_round, _ = FA.fit_from_moments(moments, "affine", trim=2.0, rounds=5)
    print("corner error per round:", " ".join(f"{e:.3g}" for e in calls), "counts:", per_round)
    assert per_round[0] == (H * W, 0, 0, 0) and calls[0] > 1.0
    assert per_round[-1] == (H * W - 1500, 0, 0, 1500) and per_round[-1] == per_round[-2] and len(per_round) < 6
    assert np.abs(FA._to_absolute(Tc, f.shape) - R.fit_ref(f, "affine", keep)).max() <= SOLVE_TOL
    assert calls[-1] < 0.05 * calls[0]
    # rounds = 0 and trim = None are the untrimmed fit
    assert FA.fit_from_moments(moments, "affine", trim=2.0, rounds=0)[1] == [per_round[0]]


def test_local_affine_maps_of_two_rotations():
    """Left half: 2 degrees and 1 % larger about its centre; right half: -1 degree, 3 % smaller, shifted.  The cells are
    the halves.  The flow is rounded to float32 (2^-24 x 8 px = 5e-7 px a pixel), which over lever arms of tens of pixels
    moves the linear part by less than 1e-7 and the shift at the centre by less than 5e-7: the bounds below are wider."""
    H, W = 64, 120
    halves = [(2.0, 1.01, (0.0, 0.0)), (-1.0, 0.97, (1.5, -0.75))]
    f = np.zeros((H, W, 2), F32)
    expect = []
    for j, (deg, sc, sh) in enumerate(halves):
        x0 = j * 60
        c = np.array([x0 + 29.5, 31.5])
        th = math.radians(deg)
        L = sc * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        T = np.concatenate([L, (c - L @ c + np.array(sh))[:, None]], 1)
        M = R.inverse(T)
        y, x = np.mgrid[0:H, x0:x0 + 60].astype(F64)
        f[:, x0:x0 + 60, 0] = x - (M[0, 0] * x + M[0, 1] * y + M[0, 2])
        f[:, x0:x0 + 60, 1] = y - (M[1, 0] * x + M[1, 1] * y + M[1, 2])
        expect.append(T)
    sums, counts, _ = R.moments_ref(f, None, (64, 60))
    for model in ("affine", "similarity"):
        maps = FA.affine_maps(sums, counts, (H, W), (64, 60), model)
        assert isinstance(maps, FlowAffineMaps) and maps.tmat.shape == (1, 2, 2, 3) and not maps.deficient.any()
        assert np.array_equal(maps.cell_bounds[0], [[0, 64, 0, 60], [0, 64, 60, 120]])
        assert np.array_equal(maps.used, [[3840, 3840]])
        for j, (deg, sc, sh) in enumerate(halves):
            assert np.abs(maps.tmat[0, j] - expect[j]).max() <= 1e-5
            assert abs(maps.rotation_deg[0, j] - deg) <= 1e-4
            assert abs(maps.scale[0, j] - sc) <= 1e-6
            assert abs(maps.anisotropy[0, j] - 1.0) <= 1e-6
            assert abs(maps.shift_x[0, j] - sh[0]) <= 1e-5 and abs(maps.shift_y[0, j] - sh[1]) <= 1e-5
            assert abs(maps.rms[0, j] - R.weighted_rms(f[:, j * 60:(j + 1) * 60])) <= 1e-9
        s = maps.summary()
        assert s["cells"] == 2 and s["cells_deficient"] == 0 and s["model"] == model
        assert abs(s["rotation_deg_range"][0] + 1.0) <= 1e-4 and abs(s["rotation_deg_range"][1] - 2.0) <= 1e-4
    # an anisotropic cell and a deficient one
    g = R.affine_flow((8, 16), [[1.25, 0, 0], [0, 1, 0]])
    w = np.array([[1, 0]], F32)
    sums, counts, _ = R.moments_ref(g, w, (8, 8))
    maps = FA.affine_maps(sums, counts, (8, 16), (8, 8), "affine")
    assert maps.deficient.tolist() == [[False, True]] and maps.used.tolist() == [[64, 0]]
    assert abs(maps.anisotropy[0, 0] - 1.25) <= 1e-12 and abs(maps.scale[0, 0] - math.sqrt(0.8)) <= 1e-12
    assert np.isnan(maps.tmat[0, 1]).all() and np.isnan(maps.rotation_deg[0, 1]) and np.isnan(maps.rms[0, 1])
    assert maps.summary()["cells_deficient"] == 1 and maps.summary()["worst_cell"] == (0, 0)


def test_arguments_are_refused_without_a_device():
    f = R.bumpy_flow((12, 20))
    T = np.array([[1, 0, 0], [0, 1, 0]], F64)
    bad_flows = [f.astype(F64), f[..., 0], f[:, :, :1], np.zeros((0, 4, 2), F32), [[1.0, 2.0]]]
    for bad in bad_flows:
        for call in (lambda b: fit_flow_affine(b), lambda b: split_flow(b), lambda b: split_flow(b, T),
                     lambda b: join_flow(T, b), lambda b: local_affine(b, 8)):
            with pytest.raises(ValueError):
                call(bad)
    for model in ("projective", None, 3):
        with pytest.raises(ValueError, match="unknown model"):
            fit_flow_affine(f, model=model)
        with pytest.raises(ValueError, match="unknown model"):
            split_flow(f, model=model)
        with pytest.raises(ValueError, match="unknown model"):
            local_affine(f, 8, model=model)
    for weight, cells in ((np.ones((12, 21), F32), None), (np.ones((12, 20), F64), None), (np.ones((2, 3), F32), None),
                          (np.ones((2, 4), F32), 8), (np.ones((12, 20), np.int16), 8), ("keep", None)):
        with pytest.raises(ValueError):
            fit_flow_affine(f, weight=weight, cell_size=cells)
        with pytest.raises(ValueError):
            split_flow(f, weight=weight, cell_size=cells)
    with pytest.raises(ValueError):
        local_affine(f, 8, weight=np.ones((3, 3), F32))
    for cells in (0, -4, (8, 0), 2.5, (8, 8, 8), None):
        with pytest.raises(ValueError):
            local_affine(f, cells)
    for cells in (0, (8, 0), 2.5):
        with pytest.raises(ValueError):
            fit_flow_affine(f, weight=np.ones((2, 3), F32), cell_size=cells)
    for trim in (0, -1.0, float("nan"), "2", True):
        with pytest.raises(ValueError, match="trim"):
            fit_flow_affine(f, trim=trim)
        with pytest.raises(ValueError, match="trim"):
            split_flow(f, trim=trim)
    for rounds in (-1, 1.5, None):
        with pytest.raises(ValueError, match="rounds"):
            fit_flow_affine(f, trim=2.0, rounds=rounds)
    for tmat in (np.eye(3), [[1, 0, 0], [0, np.nan, 0]], "T", [[1, 0], [0, 1]]):
        with pytest.raises(ValueError):
            split_flow(f, tmat)
        with pytest.raises(ValueError):
            join_flow(tmat, f)
    for singular in ([[1, 2, 0], [2, 4, 0]], [[0, 0, 1], [0, 0, 1]]):
        with pytest.raises(ValueError, match="not invertible"):
            join_flow(singular, f)
    with pytest.raises(ValueError):
        FA.solve_flow_affine(np.zeros(13))
    # a FlowGrid's arguments are refused before the grid is expanded, which is device work
    from microaligner_amd import FlowGrid
    from microaligner_amd import device
    grid = FlowGrid(np.zeros((3, 4, 2), F32), 8, (12, 20))
    expanded = []
    real = device.get_context
    FA.get_context = device.get_context = lambda *a: expanded.append(1) or real(*a)
    try:
        for call in (lambda: fit_flow_affine(grid, "projective"), lambda: fit_flow_affine(grid, trim=0),
                     lambda: fit_flow_affine(grid, rounds=-1), lambda: fit_flow_affine(grid, weight=np.ones((12, 21), F32)),
                     lambda: split_flow(grid, model="x"), lambda: split_flow(grid, np.eye(3)), lambda: split_flow(grid, trim=-1),
                     lambda: join_flow([[1, 2, 0], [2, 4, 0]], grid), lambda: join_flow(np.eye(3), grid),
                     lambda: local_affine(grid, 8, "x"), lambda: local_affine(grid, 0),
                     lambda: local_affine(grid, 8, weight=np.ones((3, 3), F32))):
            with pytest.raises(ValueError):
                call()
    finally:
        FA.get_context = device.get_context = real
    assert expanded == []


def test_the_source_hash_is_the_parents(tmp_path, monkeypatch):
    """build.source_hash() reads the files and flags it read before this source existed: the library's hash is the
    tree's, and the hash taken with the new source and its headers struck from the build's lists -- what the parent
    commit computes from the same files -- is the same, as it is after an edit of the new source."""
    before = build.source_hash()
    assert _lib.source_hash() == before
    assert "flow_affine.hip" in build.SOURCES and "microaligner_flowaffine.h" not in " ".join(build.HEADERS)
    own = [os.path.basename(h) for h in build.SOURCE_HEADERS["flow_affine.hip"]]
    assert own == ["microaligner_flowaffine.h", "microaligner_flowsmooth.h", "cell_grid.h", "weight_map.h", "moment_sums.h"]
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "flow_affine.hip"])
    monkeypatch.setattr(build, "SOURCE_HEADERS", {k: v for k, v in build.SOURCE_HEADERS.items() if k != "flow_affine.hip"})
    assert build.source_hash() == before
    monkeypatch.undo()
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc, ignore=shutil.ignore_patterns("*.o"))
    headers = [str((csrc if os.path.samefile(os.path.dirname(h), build.CSRC) else tmp_path) / os.path.basename(h))
               for h in build.HEADERS]
    shutil.copy(os.path.join(ROOT, "include", "microaligner_hip.h"), tmp_path / "microaligner_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADERS", headers)
    assert build.source_hash() == before
    with open(csrc / "flow_affine.hip", "a") as fh:
        fh.write("\n// edited\n")
    assert build.source_hash() == before
    with open(csrc / "remap.hip", "a") as fh:
        fh.write("\n// edited\n")
    assert build.source_hash() != before


def test_the_names_are_exported():
    import microaligner_amd
    for name in ("fit_flow_affine", "split_flow", "join_flow", "local_affine", "FlowAffineMaps", "FlowAffineInfo"):
        assert name in microaligner_amd.__all__ and hasattr(microaligner_amd, name)
    for name in ("ma_flow_affine_moments", "ma_flow_affine_apply"):
        assert name in _lib.FLOWAFFINE_SIGNATURES
        assert name in open(os.path.join(ROOT, "include", "microaligner_flowaffine.h")).read()
