"""-m gpu: refining a flow on the device.  ma_flow_refine_step against the numpy float32 statement of
include/microaligner_flowrefine.h (tests/_flow_refine_ref.py) bit for bit, its three statistics exactly; refine_flow()
against the statement's loop; refused arguments; the plumbing of the new header."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_refine_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402
from _remap_interp_ref import InterpRef  # noqa: E402
from microaligner_amd import FlowGrid, FlowRefineInfo, _lib, refine_flow  # noqa: E402
from microaligner_amd.device import DeviceArray, RefineStepInfo, grid_nodes  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowrefine.h")
DTYPES = [np.uint8, np.uint16, np.float32]
FULL = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}
# one tile of either pass is 64 x 128: exactly one, one past in both axes, many blocks along either axis, single lines
SHAPES = [(37, 515), (97, 161), (64, 128), (65, 129), (1, 300), (300, 1)]
RADII = {1: SHAPES, 12: SHAPES, 128: [(97, 161), (1, 300)]}


@pytest.fixture(scope="module")
def interp(tmp_path_factory):
    return InterpRef(tmp_path_factory.mktemp("remap_interp_ref"))


def taps_of(r):
    sigma = r / 3.0
    taps = R.gaussian_taps(sigma, (r - 0.5) / sigma)         # ceil(r - 0.5) = r whatever the rounding of the product
    assert len(taps) == r + 1
    return taps


def same_bits(got, exp):
    """array_equal as bit patterns, any NaN payload standing for NaN"""
    assert got.dtype == exp.dtype == F32 and got.shape == exp.shape
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(got.view(np.uint32)[~gn], exp.view(np.uint32)[~en])


def make_case(H, W, dtype, seed=0):
    """(ref of dtype, warped float32 in the same grey levels, flow): a texture under an envelope that is exactly 0 in the
    lower right part, the warped image a shifted, noisier copy, so that textured, edge and flat pixels all occur"""
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    env = np.clip(1.2 - (x / max(W - 1, 1)) ** 2 - (y / max(H - 1, 1)) ** 2, 0, 1)

    def img(dx, dy, noise):
        return 0.5 + 0.5 * env * (0.4 * np.cos((x + dx) / 3.0) * np.cos((y + dy) / 4.0) + noise * rng.random((H, W)) - 0.2)

    full = FULL[dtype]
    ref = img(0, 0, 0.2) * full
    ref = ref.astype(F32) if dtype is np.float32 else np.rint(ref).astype(dtype)
    wp = (img(0.4, -0.3, 0.25) * full).astype(F32)
    flow = rng.normal(0, 3, (H, W, 2)).astype(F32)
    return ref, wp, flow


def floor_of(dtype):
    return 1e-3 * FULL[dtype] ** 2


def check(ctx, ref, wp, flow, taps, floor, weight=None, max_step=1.0):
    """the flow with and without the statistics, out of place and in place, against the statement"""
    exp, s = R.step(ref, wp, flow, taps, floor, weight, max_step)
    d = [ctx.asdevice(a) for a in (ref, wp, flow)]
    dw = None if weight is None else ctx.asdevice(weight)
    got, info = ctx.flow_refine_step(*d, taps, floor, dw, max_step, return_info=True)
    assert isinstance(info, RefineStepInfo) and isinstance(got, DeviceArray)
    assert same_bits(got.numpy(), exp)
    assert (info.step_max, info.clamped, info.invalid) == (s.step_max, s.clamped, s.invalid), (info, s)
    assert same_bits(ctx.flow_refine_step(*d, taps, floor, dw, max_step).numpy(), exp)
    assert same_bits(d[2].numpy(), flow)                                      # the input was left alone
    inplace = d[2].copy()
    res, info2 = ctx.flow_refine_step(d[0], d[1], inplace, taps, floor, dw, max_step, return_info=True, out=inplace)
    assert res is inplace and same_bits(inplace.numpy(), exp) and info2 == info
    return exp, s


@pytest.mark.parametrize("r, shape", [(r, s) for r, shapes in RADII.items() for s in shapes])
def test_the_step_equals_the_numpy_statement_bit_for_bit(ctx, shape, r):
    """uint8, uint16 and float32 references; in place and out of place; with and without the statistics"""
    taps = taps_of(r)
    for dtype in DTYPES:
        ref, wp, flow = make_case(*shape, dtype)
        _, s = check(ctx, ref, wp, flow, taps, floor_of(dtype))
        assert s.invalid == 0


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("shape", [(37, 515), (65, 129)])
def test_weights(ctx, shape, kind):
    """a float32 weight with NaN, 0, negative and infinite entries, and a uint8 mask, which equals its 0 / 1 float map"""
    H, W = shape
    rng = np.random.default_rng(4)
    for dtype in DTYPES:
        ref, wp, flow = make_case(H, W, dtype)
        if kind == "f32":
            weight = rng.uniform(0.1, 2, (H, W)).astype(F32)
            weight[rng.random((H, W)) < 0.2] = 0
            weight[3, 5], weight[H - 1, W - 1], weight[H // 2, W // 2], weight[0, 0] = np.nan, -1.0, np.inf, -np.inf
            weight[H // 3, : W // 2] = -0.5
        else:
            weight = (rng.random((H, W)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
        exp, s = check(ctx, ref, wp, flow, taps_of(5), floor_of(dtype), weight)
        plain, _ = R.step(ref, wp, flow, taps_of(5), floor_of(dtype))
        assert not np.array_equal(exp, plain)
        if kind == "u8":
            as_map, s2 = R.step(ref, wp, flow, taps_of(5), floor_of(dtype), (weight != 0).astype(F32))
            assert np.array_equal(exp, as_map) and s == s2
    zero = np.zeros((H, W), F32 if kind == "f32" else np.uint8)
    exp, s = check(ctx, ref, wp, flow, taps_of(5), floor_of(dtype), zero)
    assert np.array_equal(exp, flow) and s == R.Stats(0.0, 0, 0)


@pytest.mark.parametrize("r", [2, 12])
def test_nan_and_inf_pixels_and_nan_flow(ctx, r):
    """NaN and Inf pixels in the reference and in the warped image drop out of the sums; NaN and Inf entries of the flow
    stay, and their pixels' steps count like any other"""
    ref, wp, flow = make_case(67, 301, np.float32)
    ref[20, 40], ref[50, 200], ref[66, 300] = np.nan, np.inf, -np.inf
    wp[10, 10], wp[30, 150], wp[0, 300], wp[66, 0] = np.nan, np.inf, -np.inf, np.nan
    flow[5, 5, 0], flow[40, 100, 1], flow[66, 300] = np.nan, np.inf, (-np.inf, np.nan)
    exp, s = check(ctx, ref, wp, flow, taps_of(r), floor_of(np.float32))
    assert s.invalid == 0 and np.isfinite(s.step_max) and (~np.isfinite(exp)).sum() == 4
    # a reference so large that the residual overflows: non-finite sums, the pixels around it are invalid
    ref[33, 77] = F32(-3e38)
    wp[33, 77] = F32(3e38)
    exp, s = check(ctx, ref, wp, flow, taps_of(r), floor_of(np.float32))
    assert s.invalid > 0 and np.array_equal(exp[33, 77], flow[33, 77])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_clamp_is_hit_on_some_pixels_and_not_on_others(ctx, dtype):
    ref, wp, flow = make_case(65, 129, dtype)
    taps, floor = taps_of(4), floor_of(dtype)
    free, s_free = R.step(ref, wp, flow, taps, floor, None, 1e30)
    d = np.abs(free - flow)
    max_step = float(np.median(d[d > 0]))
    exp, s = check(ctx, ref, wp, flow, taps, floor, None, max_step)
    assert 0 < s.clamped < 65 * 129 and s.step_max == float(F32(max_step)) and s_free.clamped == 0
    check(ctx, ref, wp, flow, taps, floor, None, 1e30)
    check(ctx, ref, wp, flow, taps, floor, None, 1e-30)


def test_denormal_sums_and_determinants(ctx):
    """an image of 3e-10 grey levels: the products are about 1e-22, the sums with them, and the determinant -- about 1e-44
    -- is a denormal of a few bits where there is texture and underflows to 0 where the image is flat (the floor's square
    does as well): those pixels are invalid.  At 1e-20 every product underflows and the floor alone decides."""
    ref, wp, flow = make_case(65, 129, np.float32)
    a, b = (ref * F32(3e-10)).astype(F32), (wp * F32(3e-10)).astype(F32)
    for floor in (1e-30, 1e-41):
        _, s = check(ctx, a, b, flow, taps_of(3), floor, None, 1e30)
        assert 0 < s.invalid < 65 * 129 and s.step_max > 0
    a, b = (ref * F32(1e-20)).astype(F32), (wp * F32(1e-20)).astype(F32)
    _, s = check(ctx, a, b, flow, taps_of(3), 1e-41)
    assert s.invalid == 65 * 129
    _, s = check(ctx, a, b, flow, taps_of(3), 1e-15)
    assert s == R.Stats(0.0, 0, 0)


# ---- refine_flow() ---------------------------------------------------------------------------------------------------------
def rotation(deg, cx, cy, tx=0.0, ty=0.0):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty]])


def e2e_pair(dtype):
    """the 97 x 161 analytic pair, the moving image smaller than the reference and seen through a rotation of 2 degrees"""
    H, W = 97, 161
    ref, mov, _ = R.analytic_pair(H, W)
    tmat = rotation(2.0, W / 2, H / 2, 0.5, -0.25)
    mov = mov[3:-2, 2:-4]
    if dtype is not np.float32:
        ref, mov = np.rint(ref).astype(dtype), np.rint(mov).astype(dtype)
    flow = np.random.default_rng(2).normal(0, 0.3, (H, W, 2)).astype(F32)
    return np.ascontiguousarray(ref), np.ascontiguousarray(mov), flow, tmat


def same_info(info, stats, converged):
    assert isinstance(info, FlowRefineInfo) and info.iterations == len(stats) == len(info.steps)
    assert info.converged == converged
    assert [tuple(s) for s in info.steps] == [tuple(s) for s in stats], (info.steps, stats)
    return True


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_refine_flow_equals_the_statements_loop(ctx, interp, dtype):
    ref, mov, flow, tmat = e2e_pair(dtype)
    exp, stats, converged = R.refine(interp, ref, mov, flow, 2.5, tmat=tmat, num_iter=3)
    got, info = refine_flow(ref, mov, flow, floor=2.5, tmat=tmat, return_info=True)
    assert isinstance(got, np.ndarray) and same_bits(got, exp) and same_info(info, stats, converged)
    assert info.iterations == 3 and not info.converged and not np.array_equal(got, flow)
    # without the statistics: the same flow; device arrays in, a device array out, the caller's flow untouched
    assert same_bits(refine_flow(ref, mov, flow, floor=2.5, tmat=tmat), exp)
    d_flow = ctx.asdevice(flow).copy()
    d_got = refine_flow(ctx.asdevice(ref), ctx.asdevice(mov), d_flow, floor=2.5, tmat=tmat)
    assert isinstance(d_got, DeviceArray) and d_got is not d_flow and same_bits(d_got.numpy(), exp)
    assert same_bits(d_flow.numpy(), flow)
    # no flow: zeros, the kind of the reference; no matrix: the identity
    same = np.ascontiguousarray(R.analytic_pair(97, 161)[1].astype(dtype))
    exp0, stats0, conv0 = R.refine(interp, ref, same, None, 2.5, num_iter=2, sigma=2.0, max_step=0.25)
    got0, info0 = refine_flow(ctx.asdevice(ref), same, floor=2.5, num_iter=2, sigma=2.0, max_step=0.25, return_info=True)
    assert isinstance(got0, DeviceArray) and same_bits(got0.numpy(), exp0) and same_info(info0, stats0, conv0)
    assert info0.steps[0].clamped > 0
    # tol: the loop stops after the first step within it
    tol = stats[1].step_max
    exp_t, stats_t, conv_t = R.refine(interp, ref, mov, flow, 2.5, tmat=tmat, num_iter=3, tol=tol)
    got_t, info_t = refine_flow(ref, mov, flow, floor=2.5, tmat=tmat, tol=tol, return_info=True)
    assert same_bits(got_t, exp_t) and same_info(info_t, stats_t, conv_t) and info_t.converged and info_t.iterations <= 2
    assert same_bits(refine_flow(ref, mov, flow, floor=2.5, tmat=tmat, tol=tol), exp_t)


def test_refine_flow_with_a_weight_and_a_flow_grid(ctx, interp):
    ref, mov, flow, tmat = e2e_pair(np.float32)
    mask = np.ones(ref.shape, np.uint8)
    mask[:, :40] = 0
    exp, stats, converged = R.refine(interp, ref, mov, flow, 2.5, tmat=tmat, num_iter=2, weight=mask)
    got, info = refine_flow(ref, mov, flow, floor=2.5, tmat=tmat, num_iter=2, weight=mask, return_info=True)
    assert same_bits(got, exp) and same_info(info, stats, converged)
    # a FlowGrid is its expansion; numpy nodes give numpy, device nodes a DeviceArray
    nodes = np.random.default_rng(3).normal(0, 0.4, (grid_nodes(97, 16), grid_nodes(161, 16), 2)).astype(F32)
    grid = FlowGrid(nodes, 16, ref.shape)
    dense = grid.expand()
    assert isinstance(dense, np.ndarray)
    exp, stats, converged = R.refine(interp, ref, mov, dense, 2.5, tmat=tmat, num_iter=2)
    got, info = refine_flow(ref, mov, grid, floor=2.5, tmat=tmat, num_iter=2, return_info=True)
    assert isinstance(got, np.ndarray) and same_bits(got, exp) and same_info(info, stats, converged)
    assert same_bits(refine_flow(ref, mov, dense, floor=2.5, tmat=tmat, num_iter=2), exp)
    d_got = refine_flow(ref, mov, FlowGrid(ctx.asdevice(nodes), 16, ref.shape), floor=2.5, tmat=tmat, num_iter=2)
    assert isinstance(d_got, DeviceArray) and same_bits(d_got.numpy(), exp)


def test_dog_labels_are_the_gates(ctx, interp):
    ref, mov, flow, tmat = e2e_pair(np.float32)
    l_ref, l_mov = (ctx.dog_u8(ctx.asdevice(a), 5, 9).numpy() for a in (ref, mov))
    assert l_ref.dtype == np.uint8 and l_mov.shape == mov.shape
    exp, stats, converged = R.refine(interp, l_ref, l_mov, flow, 4.0, tmat=tmat, num_iter=3)
    got, info = refine_flow(ref, mov, flow, floor=4.0, tmat=tmat, labels="dog", return_info=True)
    assert same_bits(got, exp) and same_info(info, stats, converged)
    assert same_bits(refine_flow(l_ref, l_mov, flow, floor=4.0, tmat=tmat), exp)


# ---- refused arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_c_entry(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    ref, wp, flow = make_case(H, W, np.uint8)
    d_ref, d_wp, d_flow, d_out = ctx.asdevice(ref), ctx.asdevice(wp), ctx.asdevice(flow), ctx.asdevice(np.full((H, W, 2), 7, F32))
    d_w = ctx.asdevice(np.ones((H, W), F32))
    stats = (C.c_longlong * 3)()
    taps = (C.c_float * 4)(0.4, 0.2, 0.1, 0.0)

    def bad_taps(*v):
        return (C.c_float * len(v))(*v)
    ok = dict(ref=d_ref.ptr, dtype=0, wp=d_wp.ptr, H=H, W=W, taps=taps, r=3, floor=50.0, weight=d_w.ptr, kind=1, max_step=1.0,
              flow=d_flow.ptr, out=d_out.ptr, stats=stats)
    step = lambda **kw: ctx._run(ctx.lib.ma_flow_refine_step, *dict(ok, **kw).values())     # noqa: E731
    step()
    exp, s = R.step(ref, wp, flow, np.array(taps[:], F32), 50.0, np.ones((H, W), F32))
    assert same_bits(d_out.numpy(), exp)
    assert (stats[0], stats[1]) == (s.invalid, s.clamped)
    assert float(np.array([stats[2]], np.uint32).view(F32)[0]) == s.step_max
    step(weight=None, kind=0, stats=None)            # the weight is read only for a kind that has one
    for kw in (dict(ref=None), dict(wp=None), dict(taps=None), dict(flow=None), dict(out=None), dict(weight=None),
               dict(H=0), dict(W=0), dict(H=-1), dict(H=big), dict(W=big), dict(r=0), dict(r=-1), dict(r=129),
               dict(dtype=3), dict(dtype=-1), dict(kind=3), dict(kind=-1), dict(kind=4),
               dict(taps=bad_taps(0.0, 0.2, 0.1, 0.0)), dict(taps=bad_taps(0.4, -0.2, 0.1, 0.0)),
               dict(taps=bad_taps(0.4, 0.2, float("nan"), 0.0)), dict(taps=bad_taps(0.4, 0.2, 0.1, float("inf"))),
               dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")),
               dict(max_step=0.0), dict(max_step=-1.0), dict(max_step=float("nan")), dict(max_step=float("inf")),
               dict(out=d_ref.ptr), dict(out=d_wp.ptr), dict(out=d_w.ptr)):
        with pytest.raises(ValueError):
            step(**kw)
    assert ctx.lib.ma_flow_refine_step(None, *ok.values()) == _lib.MA_EINVAL
    ctx.sync()
    exp, _ = R.step(ref, wp, flow, np.array(taps[:], F32), 50.0)
    assert same_bits(d_out.numpy(), exp)             # a refused call wrote nothing
    with pytest.raises(ValueError):
        ctx.flow_refine_step(d_ref, d_wp, d_flow, np.array(taps[:], F32), 50.0, out=ctx.asdevice(np.zeros((H, W), F32)))


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    import microaligner_amd
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_flow_refine_step"] == sorted(_lib.FLOWREFINE_SIGNATURES)
    assert hasattr(lib, "ma_flow_refine_step"), "ma_flow_refine_step declared in microaligner_flowrefine.h but not exported"
    proto = re.search(r"\bma_flow_refine_step\s*\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.FLOWREFINE_SIGNATURES["ma_flow_refine_step"][1])
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES, _lib.FLOWCOMPOSE_SIGNATURES,
              _lib.FLOWINVERT_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.FLOWGRID_SIGNATURES, _lib.FLOWSMOOTH_SIGNATURES,
              _lib.FLOWAFFINE_SIGNATURES, _lib.TEXTURE_SIGNATURES, _lib.DIRECT_SIGNATURES]
    assert not any(set(_lib.FLOWREFINE_SIGNATURES) & set(t) for t in others)
    consts = re.findall(r"#define\s+(MA_[A-Z0-9_]+)\s+(\d+)\b", text)
    assert sorted(n for n, _ in consts) == ["MA_REFINE_MAX_RADIUS", "MA_REFINE_STATS"]
    for name, value in consts:
        assert getattr(_lib, name) == int(value), name
    assert _lib.MA_REFINE_MAX_RADIUS == _lib.MA_SMOOTH_MAX_RADIUS       # one check of the taps serves both
    assert {"refine_flow", "FlowRefineInfo"} <= set(microaligner_amd.__all__)


def test_the_source_hash_is_the_parents():
    from microaligner_amd import build
    assert build.source_hash() == HASH == _lib.source_hash()
    assert "flow_refine.hip" in build.SOURCES and "microaligner_flowrefine.h" not in " ".join(build.HEADERS)
    assert [os.path.basename(h) for h in build.SOURCE_HEADERS["flow_refine.hip"]] == ["microaligner_flowrefine.h",
                                                                                      "microaligner_flowsmooth.h",
                                                                                      "window_fir.h", "weight_map.h",
                                                                                      "call_counts.h"]
