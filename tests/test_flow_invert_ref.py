"""The flow inverse and the point transforms on the CPU (no GPU): the numpy statements of
include/microaligner_flowinvert.h (tests/_flow_invert_ref.py) held to bounds derived from the inputs -- the Lipschitz
constant of the flow array, the tolerances, the number formats -- never from the code under test; identities; argument
checks before any device work; the plumbing of the new header."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_compose_ref as RC  # noqa: E402
import _flow_invert_ref as R  # noqa: E402
from microaligner_amd.device import affine_flow_params  # noqa: E402

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowinvert.h")
MAX_ITER = 60
_CACHE = {}


def flow(name):
    if name not in _CACHE:
        _CACHE[name] = R.analytic_flow(name)
    return _CACHE[name]


def inverse(name, tol):
    if (name, tol) not in _CACHE:
        _CACHE[name, tol] = R.invert_flow_ref(flow(name), MAX_ITER, tol)
    return _CACHE[name, tol]


def test_lipschitz_constants_of_the_test_flows():
    """the arrays' constants are the analytic ones up to the sampling (A 0.273, B 0.508, C 0.666, F 1.33)"""
    got = {n: R.lipschitz(flow(n)) for n in "ABCF"}
    print(got)
    for n, exp in (("A", 0.273), ("B", 0.508), ("C", 0.666), ("F", 1.33)):
        assert abs(got[n] - exp) < 0.005
    for n in "ABC":
        assert got[n] <= R.ANALYTIC[n][2] + 1e-6 < 1


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_every_pixel_of_a_contracting_flow_converges(name, tol):
    g, res, missed, steps = inverse(name, tol)
    print(f"{name} tol={tol}: steps mean {steps.mean():.2f} max {steps.max()}, residual max {res.max():.3g}")
    assert missed == 0 and steps.max() < MAX_ITER and res.max() <= F32(tol)


def test_a_folding_flow_does_not_converge_everywhere():
    g, res, missed, steps = R.invert_flow_ref(flow("F"), MAX_ITER, 1e-3)
    print(f"F: not converged {missed} of {steps.size}")
    assert missed > 0 and missed == int(((steps == MAX_ITER) & ~(res <= F32(1e-3))).sum())


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_composition_with_the_inverse_is_zero_within_the_derived_bound(name, tol):
    """compose(f, g)(q) = g(q) + f sampled at q - g(q) by compose_flows' sampler.  g(q) = -S(q - g_prev(q)) with
    |g - g_prev| <= tol, and the quantised sampler moves the coordinate by at most 1/64 px per axis: the two samples of
    f lie within 1/64 + tol per axis, so differ by at most L (1/64 + tol); 1e-4 for the float32 rounding of flows below
    32 px.  Nothing is asserted on compose(g, f), which g's own Lipschitz constant governs."""
    f = flow(name)
    g = inverse(name, tol)[0]
    L = R.lipschitz(f)
    got = float(np.abs(RC.compose_flows_ref(f, g)).max())
    bound = L * (1 / 64 + tol) + 1e-4
    print(f"{name} tol={tol}: max |compose(f, g)| = {got:.5f} px, bound {bound:.5f} px")
    assert got <= bound


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_within_the_derived_bound_of_the_analytic_inverse(name, tol):
    """truth g*(q) = q - p*, p* - f(p*) = q on the analytic flow in float64.  The statement iterates the bilinear
    interpolant, which is within E of the analytic flow, and stops within tol of its own fixed point: a contraction with
    constant La turns a defect of E + La tol into an error of at most (E + La tol) / (1 - La); 1e-4 for float32."""
    g = inverse(name, tol)[0]
    truth, inside = R.analytic_inverse(name)
    La, E = R.ANALYTIC[name][2:]
    got = float(np.abs(g.astype(F64) - truth)[inside].max())
    bound = (E + La * tol) / (1 - La) + 1e-4
    print(f"{name} tol={tol}: max |g - g*| = {got:.5f} px over {inside.mean():.3f} of the image, bound {bound:.5f} px")
    assert inside.mean() > 0.9 and got <= bound


def random_points(n, seed, H, W, margin):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-margin, W - 1 + margin, n), rng.uniform(-margin, H - 1 + margin, n)], -1)


TMAT = np.array([[np.cos(np.deg2rad(3.0)) * 1.01, -np.sin(np.deg2rad(3.0)) * 1.01, 7.5],
                 [np.sin(np.deg2rad(3.0)) * 1.01, np.cos(np.deg2rad(3.0)) * 1.01, -4.25]])


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_points_round_trip_within_l_tol(name):
    """p = to_reference(q) ends with p = q + S(p_prev), |p - p_prev| <= tol, and to_moving(p) = p - S(p), so the round
    trip is off by S(p_prev) - S(p): at most L tol; 1e-9 for the float64 roundings.  Points outside the image included:
    the clamp does not raise the Lipschitz constant."""
    f, tol = flow(name), 1e-4
    H, W = f.shape[:2]
    L = R.lipschitz(f)
    q = random_points(200000, 3, H, W, 30.0)
    p, conv, inside, steps = R.to_reference_ref(q, f, max_iter=MAX_ITER, tol=tol)
    back, conv2, inside2 = R.to_moving_ref(p, f)
    err = float(np.abs(back - q).max())
    print(f"{name}: round trip max {err:.4g} px, bound {L * tol + 1e-9:.4g} px, steps mean {steps.mean():.2f} max {steps.max()}")
    assert conv.all() and conv2.all() and np.array_equal(inside, inside2) and 0 < inside.mean() < 1
    assert err <= L * tol + 1e-9


@pytest.mark.parametrize("name", ["A", "C"])
def test_points_round_trip_through_tmat_and_padding(name):
    """with a matrix: to_reference solves p - S(p) = a = T (s + pad) up to L tol as above, and to_moving returns
    M (p - S(p)) - pad with M = T^-1: off by at most |M|_inf L tol; 1e-9 for the roundings at coordinates below 2^10."""
    f, tol = flow(name), 1e-4
    H, W = f.shape[:2]
    shape = (H - 21, W - 10)
    _, m6, left, top = affine_flow_params(shape, F32, f.shape, f.dtype, TMAT)
    assert (left, top) == (5, 10)
    s = random_points(100000, 4, shape[0], shape[1], 10.0)
    p, conv, _, _ = R.to_reference_ref(s, f, TMAT.ravel(), (left, top), MAX_ITER, tol)
    back, _, _ = R.to_moving_ref(p, f, m6, (left, top))
    norm = float(np.abs(np.asarray(m6).reshape(2, 3)[:, :2]).sum(1).max())
    err, bound = float(np.abs(back - s).max()), norm * R.lipschitz(f) * tol + 1e-9
    print(f"{name}: round trip through tmat max {err:.4g} px, bound {bound:.4g} px")
    assert conv.all() and err <= bound


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_dense_inverse_and_points_agree_at_integer_pixels(name):
    """q - g(q) and to_reference(q) both solve p - f(p) = q: the first within L tol_dense of its fixed-point equation in
    float32 arithmetic (coordinates below max(H, W) carry 2^-24 relative rounding, 8 operations), the second within
    L tol_pts; a contraction divides the defect by 1 - L."""
    f = flow(name)
    H, W = f.shape[:2]
    tol_dense, tol_pts = 1e-3, 1e-4
    g = inverse(name, tol_dense)[0]
    L = R.lipschitz(f)
    ys, xs = np.mgrid[0:H:7, 0:W:5]
    q = np.stack([xs.ravel(), ys.ravel()], -1).astype(F64)
    p, conv, _, _ = R.to_reference_ref(q, f, max_iter=MAX_ITER, tol=tol_pts)
    dense = q - g[ys.ravel(), xs.ravel()].astype(F64)
    err = float(np.abs(dense - p).max())
    bound = (L * (tol_dense + tol_pts) + 8 * 2.0 ** -24 * max(H, W)) / (1 - L)
    print(f"{name}: max |(q - g(q)) - to_reference(q)| = {err:.4g} px, bound {bound:.4g} px")
    assert conv.all() and err <= bound


def test_identities():
    z = np.zeros((37, 53, 2), F32)
    g, res, missed, steps = R.invert_flow_ref(z, 5, 0.0)
    assert np.array_equal(g, z) and missed == 0 and steps.max() == 1 and not res.any()
    c = np.empty_like(z)
    c[...] = (3.0, -7.0)                                  # an integer shift: the samples fall on pixels
    g, res, missed, steps = R.invert_flow_ref(c, 5, 0.0)
    assert np.array_equal(g, -c) and missed == 0 and steps.min() == steps.max() == 2 and not res.any()
    # max_iter = 1 takes the one step and reports every pixel whose step was larger than tol
    g, res, missed, steps = R.invert_flow_ref(c, 1, 1e-3)
    assert np.array_equal(g, -c) and missed == c.shape[0] * c.shape[1] and np.array_equal(res, np.full(c.shape[:2], F32(7)))
    pts = np.array([[4.0, 5.0], [0.5, 36.0], [-3.0, 2.0], [52.0, 36.0], [52.5, 1.0]])
    out, conv, inside = R.to_moving_ref(pts, c)
    assert np.array_equal(out, pts - (3.0, -7.0)) and conv.all() and inside.tolist() == [1, 1, 0, 1, 0]
    out, conv, inside, steps = R.to_reference_ref(pts, c, max_iter=5, tol=0.0)
    assert np.array_equal(out, pts + (3.0, -7.0)) and conv.all() and steps.max() == 2
    assert inside.tolist() == [0, 1, 0, 0, 0]             # the registered-frame coordinate, i.e. the result


def test_non_finite_values_stay_local():
    """a non-finite value of f reaches the pixels whose iterates sample it -- within max |f| + 1 px of it -- and no
    others; a non-finite point gives NaN, not converged, not inside, and leaves the other points alone."""
    f = R.analytic_flow("A", (120, 160))
    clean = R.invert_flow_ref(f, 40, 1e-4)
    bad = f.copy()
    bad[60, 80] = (np.nan, 1.0)
    bad[20, 30] = (np.inf, -np.inf)
    bad[100, 140] = (1e30, -1e30)
    g, res, missed, steps = R.invert_flow_ref(bad, 40, 1e-4)
    reach = float(np.abs(f).max()) + 1
    y, x = np.mgrid[0:120, 0:160]
    near = np.zeros((120, 160), bool)
    for py, px in ((60, 80), (20, 30), (100, 140)):
        near |= (np.abs(y - py) <= reach) & (np.abs(x - px) <= reach)
    changed = ~((g == clean[0]).all(-1) & (res == clean[1]))
    assert changed.any() and not (changed & ~near).any()
    assert missed == int((np.isnan(res) | (res > F32(1e-4))).sum()) and missed > 0
    assert np.isnan(res[np.isnan(g).any(-1)]).all()
    pts = np.array([[10.0, 10.0], [np.nan, 3.0], [5.0, np.inf], [-np.inf, np.nan], [100.5, 50.25]])
    for out, conv, inside in (R.to_moving_ref(pts, f), R.to_reference_ref(pts, f)[:3]):
        assert np.isnan(out[1:4]).all() and not conv[1:4].any() and not inside[1:4].any()
        assert np.isfinite(out[[0, 4]]).all() and conv[[0, 4]].all()
    ref = R.to_reference_ref(pts[[0, 4]], f)
    assert np.array_equal(R.to_reference_ref(pts, f)[0][[0, 4]], ref[0])


# ---- argument checks before any device work -----------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import microaligner_amd.optflow_reg.flow_invert as mod

    def refuse(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(mod, "get_context", refuse)


FLOW = np.zeros((8, 9, 2), F32)
PTS = np.zeros((4, 2), F64)


@pytest.mark.parametrize("kw", [dict(flow=FLOW.astype(F64)), dict(flow=FLOW[..., 0]), dict(flow=np.zeros((8, 9, 3), F32)),
                                dict(flow=np.zeros((0, 9, 2), F32)), dict(flow=[[0.0, 0.0]]), dict(max_iter=0),
                                dict(max_iter=-1), dict(max_iter=2.5), dict(max_iter=True), dict(max_iter=None),
                                dict(tol=-1e-3), dict(tol=np.nan), dict(tol=np.inf), dict(tol=1e39), dict(tol="1e-3"),
                                dict(tol=None)])
def test_invert_flow_refuses_bad_arguments_before_device_work(no_device, kw):
    from microaligner_amd import invert_flow
    with pytest.raises(ValueError):
        invert_flow(**dict(dict(flow=FLOW), **kw))


@pytest.mark.parametrize("kw", [dict(points=PTS.astype(F32)), dict(points=np.zeros((4, 3))), dict(points=np.zeros(4)),
                                dict(points=[[1.0, 2.0]]), dict(points=np.zeros((4, 2), np.int64)),
                                dict(flow=FLOW.astype(F64)), dict(flow=FLOW[..., 0]), dict(direction="forward"),
                                dict(direction="TO_MOVING"), dict(direction=None), dict(direction=0), dict(max_iter=0),
                                dict(max_iter=1.0), dict(tol=-1.0), dict(tol=np.nan), dict(tol=np.inf), dict(tol=None),
                                dict(tmat=np.eye(3)), dict(tmat=[[1, 0, np.nan], [0, 1, 0]]), dict(tmat="x"),
                                dict(image_shape=(8, 9)), dict(tmat=np.eye(2, 3), image_shape=(9, 9)),
                                dict(tmat=np.eye(2, 3), image_shape=(8,)), dict(tmat=np.eye(2, 3), image_shape=(0, 4)),
                                dict(tmat=np.eye(2, 3), image_shape="ab")])
def test_transform_points_refuses_bad_arguments_before_device_work(no_device, kw):
    from microaligner_amd import transform_points
    with pytest.raises(ValueError):
        transform_points(**dict(dict(points=PTS, flow=FLOW, direction="to_moving"), **kw))


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))


def test_header_library_and_bindings_agree():
    import microaligner_amd
    from microaligner_amd import build, _lib
    build.build()
    lib = _lib.load()
    text, names = _declared(HEADER)
    assert names == ["ma_invert_flow", "ma_transform_points"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_flowinvert.h but not exported"
        proto = re.search(r"\b" + n + r"\s*\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.FLOWINVERT_SIGNATURES[n][1]), n
    assert sorted(_lib.FLOWINVERT_SIGNATURES) == names
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES,
              _lib.FLOWCOMPOSE_SIGNATURES]
    assert not any(set(_lib.FLOWINVERT_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_hip.h"' in open(HEADER).read()
    assert {"invert_flow", "transform_points"} <= set(microaligner_amd.__all__)
    assert callable(microaligner_amd.invert_flow) and callable(microaligner_amd.transform_points)
    # the C entries refuse what the header says they refuse, before they touch a device (a NULL ctx comes first)
    assert lib.ma_invert_flow(None, None, 4, 4, 5, 1e-3, None, None, None) == _lib.MA_EINVAL
    assert lib.ma_transform_points(None, None, 0, None, 4, 4, None, None, 0, 0, 0, 5, 1e-4, None, None, None) == _lib.MA_EINVAL


def test_flow_invert_stays_out_of_the_measured_path_hash(tmp_path, monkeypatch):
    from microaligner_amd import build
    assert "flow_invert.hip" in build.SOURCES and HEADER not in [os.path.abspath(h) for h in build.HEADERS]
    assert [os.path.abspath(h) for h in build.SOURCE_HEADERS["flow_invert.hip"]] == [HEADER,
                                                                                     os.path.join(build.CSRC, "call_counts.h")]
    before = build.source_hash()
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc)
    headers = [str((csrc if os.path.samefile(os.path.dirname(h), build.CSRC) else tmp_path) / os.path.basename(h))
               for h in build.HEADERS]
    shutil.copy(os.path.join(ROOT, "include", "microaligner_hip.h"), tmp_path / "microaligner_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADERS", headers)
    assert build.source_hash() == before
    with open(csrc / "flow_invert.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() == before
    with open(csrc / "remap.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() != before
