"""-m gpu: the affine moments of a flow and apply(flow, A) on the device against the numpy statement of
include/microaligner_flowaffine.h (tests/_flow_affine_ref.py) -- counts exactly, sums within the bound every order of
summation keeps, apply bit for bit -- and the entry points end to end."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_affine_ref as R  # noqa: E402
from microaligner_amd import FlowAffineInfo, FlowGrid, _lib, fit_flow_affine, join_flow, local_affine, split_flow, \
    transform_points  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402
from microaligner_amd.optflow_reg import flow_affine as FA  # noqa: E402
from test_flow_affine_ref import SOLVE_TOL, rotation_flow  # noqa: E402
from test_gpu_flow_invert import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowaffine.h")

# 96 x 161: an odd width, so rows are not 16-byte aligned; 65 x 511: one more row and one more column than the moments
# tile (64 rows x 510 columns); the degenerate ones
SHAPES = [(96, 161), (65, 511), (1, 64), (64, 1), (2, 3), (1, 1)]
U = 2.0 ** -53
# the end-to-end tolerance: the CPU test's, times 4 for the other order of summation (the spread between orders measured
# in test_flow_affine_ref.test_the_order_of_summation_moves_the_fit_by_less_than_the_gpu_factor is 1.6e-13)
E2E_TOL = 4 * SOLVE_TOL


def make_flow(H, W, odd=False):
    rng = np.random.default_rng(1000 * H + W)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    f = np.stack([3 * np.sin(x / 17) + 2 * np.cos(y / 23) + 0.02 * x, 2.5 * np.cos(x / 13 + y / 31) - 0.01 * y], -1)
    f = (f + rng.normal(0, 0.3, (H, W, 2))).astype(F32)
    if odd:
        vals = ((np.nan, 1.0), (np.inf, -np.inf), (-np.inf, np.nan), (2.0, np.nan), (np.inf, 0.5), (1e3, -1e3))
        for k, v in enumerate(vals):
            f[(5 + 11 * k) % H, (6 + 37 * k) % W] = v
    return f, rng


def make_weight(kind, H, W, rng, cells):
    if kind == "none":
        return None
    if kind == "f32":
        w = rng.uniform(0.25, 2.0, (H, W)).astype(F32)
        w[rng.random((H, W)) < 0.3] = 0
        for k, v in enumerate((np.nan, -1.0, 0.0, np.inf, -np.inf, -0.0, 1e-40)):
            w[(3 + 7 * k) % H, (2 + 29 * k) % W] = v
        return w
    if kind == "u8":
        return (rng.random((H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
    gy, gx = -(-H // cells[0]), -(-W // cells[1])
    return np.resize(np.array([1.0, 0.5, np.nan, 2.0, -2.0, 1.5, 0.0, 0.75, np.inf], F32), (gy, gx))


def check_moments(ctx, f, weight, cells, prior=None, clip=None):
    """counts equal; every sum within (n + 1) 2^-53 sum |term| of the fsum; a second call gives the same bits"""
    exp, exp_counts, exp_abs = R.moments_ref(f, weight, cells, prior, clip)
    d, dw = ctx.asdevice(f), None if weight is None else ctx.asdevice(weight)
    sums, counts = ctx.flow_affine_moments(d, dw, cells, prior, clip)
    assert sums.shape == exp.shape and sums.dtype == F64 and counts.dtype == np.int64
    assert np.array_equal(counts, exp_counts)
    H, W = f.shape[:2]
    areas = [[(s[0].stop - s[0].start) * (s[1].stop - s[1].start) for s in row] for row in R.cell_slices((H, W), cells)]
    assert np.array_equal(counts.sum(-1), areas)
    bound = (exp_counts[..., :1] + 1) * U * exp_abs
    err = np.abs(sums - exp)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    assert np.all(sums[exp_counts[..., 0] == 0] == 0.0)
    again = ctx.flow_affine_moments(d, dw, cells, prior, clip)
    assert np.array_equal(again[0].view(np.uint64), sums.view(np.uint64)) and np.array_equal(again[1], counts)
    return sums, counts, exp, exp_counts, exp_abs


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_equal_the_statement(ctx, shape):
    """every weight kind x one cell, ragged (32, 50) cells and a cell larger than the image; flows with NaN / Inf pixels;
    the per-cell sums add up to the one-cell sums"""
    H, W = shape
    f, rng = make_flow(H, W, odd=H * W > 100)
    grids = [None, (32, 50), (200, 600)] + ([1] if shape == (2, 3) else [])
    for kind in ("none", "f32", "u8", "cells"):
        one = None
        for cells in grids:
            if kind == "cells" and cells is None:
                continue
            cells = (cells, cells) if isinstance(cells, int) else cells
            weight = make_weight(kind, H, W, np.random.default_rng(7), cells)
            sums, counts, exp, exp_counts, exp_abs = check_moments(ctx, f, weight, cells)
            if kind == "cells":
                continue                       # the weight map changes with the grid: nothing to add up
            if cells is None:
                one = (exp[0, 0], exp_counts[0, 0], exp_abs[0, 0])
                continue
            assert np.array_equal(counts.sum((0, 1)), one[1])
            total = np.array([math.fsum(sums[..., k].ravel()) for k in range(14)])
            assert np.all(np.abs(total - one[0]) <= (one[1][0] + 1) * U * one[2])


def test_moments_with_a_prior_trim(ctx):
    """a prior in the centred frame and a clip: identity (clips on the flow itself), a matrix near the fit, and clips
    that take everything and nothing; with weights and cells"""
    f, rng = make_flow(96, 161, odd=True)
    ident = np.array([[1, 0, 0], [0, 1, 0]], F64)
    near = np.array([[1.02, 0.003, -0.4], [-0.002, 0.99, 0.3]])
    w = make_weight("f32", 96, 161, rng, None)
    seen = set()
    for prior, clip in ((ident, 3.0), (near, 1.5), (near, 1e-9), (ident, 1e9), (near, float("inf"))):
        for weight, cells in ((None, None), (w, None), (w, (32, 50)), (make_weight("cells", 96, 161, rng, (32, 50)), (32, 50))):
            counts = check_moments(ctx, f, weight, cells, prior, clip)[1]
            seen.add((int(counts[..., 0].sum()) > 0, int(counts[..., 3].sum()) > 0))
    assert seen == {(True, True), (False, True), (True, False)}
    f2, _ = make_flow(65, 511)
    check_moments(ctx, f2, None, None, near, 2.0)


def test_moments_of_an_unaligned_flow_and_many_cells(ctx):
    """a flow 8 bytes off a 16-byte boundary takes the 8-byte loads throughout; cells of one pixel; a grid of more cells
    than rows of a tile"""
    f, _ = make_flow(40, 73, odd=True)
    base = ctx.asdevice(np.concatenate([np.zeros((1, 2), F32), f.reshape(-1, 2)]))
    view = DeviceArray(ctx, f.shape, F32, base.ptr + 8, 0, owner=False)
    exp, exp_counts, exp_abs = R.moments_ref(f, None, (16, 30))
    sums, counts = ctx.flow_affine_moments(view, None, (16, 30))
    assert np.array_equal(counts, exp_counts)
    assert np.all(np.abs(sums - exp) <= (exp_counts[..., :1] + 1) * U * exp_abs)
    aligned = ctx.flow_affine_moments(ctx.asdevice(f), None, (16, 30))
    assert np.array_equal(aligned[1], counts)
    g, _ = make_flow(9, 14)
    check_moments(ctx, g, None, (1, 1))
    check_moments(ctx, g, make_weight("cells", 9, 14, None, (1, 1)), (1, 1))


def test_a_flow_past_2_31_floats_is_indexed_in_64_bits(ctx):
    """16400 x 65600, the smallest such shape that crosses 2^31 floats (its last 32 rows lie past them; 8.6 GB), made on
    the device: apply(0, A) with A = diag(1 + 2^-10) is the flow (-x / 1024, -y / 1024), exact in float32.  With the
    identity as the prior, rho = (u, v) exactly, so clip = 10 uses the pixels with x <= 10240 and y <= 10240 and trims the
    rest: the counts per cell of 4096 are known exactly, and so are sum w, sum wX and sum wY, whose partial sums are
    half-integers below 2^53 in any order.  A 32-bit float index would wrap by 2^30 pixels = 16368 rows and 1024 columns:
    apply would leave the last rows 0, and the moments would read rows near the top there, both of which turn trimmed
    pixels of the last row of cells into used ones.  No host array of that size is made; measured on MI355X: under 0.05 s (a memset and three passes over
    8.6 GB)."""
    H, W, cell, edge = 16400, 65600, 4096, 10240
    flow = ctx.zeros((H, W, 2), F32)
    A = np.array([[1 + 2.0 ** -10, 0, 0], [0, 1 + 2.0 ** -10, 0]])
    assert ctx.flow_affine_apply(flow, A, out=flow) is flow
    sums, counts = ctx.flow_affine_moments(flow, None, cell, np.array([[1, 0, 0], [0, 1, 0]], F64), 10.0)
    y0, x0 = np.arange(0, H, cell), np.arange(0, W, cell)
    y1, x1 = np.minimum(y0 + cell, H), np.minimum(x0 + cell, W)
    ny, nx = np.clip(edge + 1 - y0, 0, y1 - y0), np.clip(edge + 1 - x0, 0, x1 - x0)     # used rows / columns per cell
    used = ny[:, None] * nx[None, :]
    area = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    assert np.array_equal(counts[..., 0], used) and np.array_equal(counts[..., 3], area - used)
    assert not counts[..., 1].any() and not counts[..., 2].any()
    sx = nx * x0 + nx * (nx - 1) / 2.0 - nx * (W - 1) / 2.0          # sum of X over a cell's used columns
    sy = ny * y0 + ny * (ny - 1) / 2.0 - ny * (H - 1) / 2.0
    assert np.array_equal(sums[..., 0], used.astype(F64))
    assert np.array_equal(sums[..., 6], ny[:, None] * sx[None, :]) and np.array_equal(sums[..., 7], sy[:, None] * nx[None, :])
    del flow


@pytest.mark.parametrize("shape", SHAPES + [(3, 700)])
def test_apply_equals_the_statement_bit_for_bit(ctx, shape):
    """split with a matrix, join with its inverse, out of place and in place; non-finite pixels propagate"""
    f, _ = make_flow(*shape, odd=shape[0] * shape[1] > 100)
    T = np.array([[1.013, -0.052, 3.25], [0.049, 0.991, -1.75]])
    for A in (T, R.inverse(T), np.array([[1, 0, 0], [0, 1, 0]], F64)):
        exp = R.apply_ref(f, A)
        d = ctx.asdevice(f)
        out = ctx.flow_affine_apply(d, A)
        assert out is not d and same_bits(out.numpy(), exp) and same_bits(d.numpy(), f)
        buf = ctx.asdevice(f.copy())
        assert ctx.flow_affine_apply(buf, A, out=buf) is buf and same_bits(buf.numpy(), exp)
    if shape[0] * shape[1] > 100:
        assert np.isnan(exp).any()


def test_fit_returns_the_exact_and_the_lstsq_matrix(ctx):
    for shape in ((37, 515), (96, 161)):
        f = R.affine_flow(shape, R.DYADIC_AFFINE)
        got = fit_flow_affine(f)
        assert got.shape == (2, 3) and got.dtype == F64
        dev = float(np.abs(got - R.inverse(R.DYADIC_AFFINE)).max())
        print(f"dyadic affine {shape}: deviation from the exact matrix {dev:.3g}")
        assert dev <= E2E_TOL
    f = R.affine_flow((96, 161), R.DYADIC_SIMILARITY)
    for model in ("affine", "similarity"):
        assert np.abs(fit_flow_affine(f, model) - R.inverse(R.DYADIC_SIMILARITY)).max() <= E2E_TOL
    f = R.bumpy_flow()
    for model in R.MODELS:
        got, info = fit_flow_affine(f, model, return_info=True)
        dev = float(np.abs(got - R.fit_ref(f, model)).max())
        print(f"bumpy {model}: deviation from the independent fit {dev:.3g}")
        assert dev <= E2E_TOL
        assert isinstance(info, FlowAffineInfo) and info.counts == [(97 * 161, 0, 0, 0)] and info.model == model
        assert abs(info.rms - R.weighted_rms(f)) <= 1e-12 * info.rms
        assert np.abs(FA._to_absolute(info.centred, f.shape) - got).max() == 0
    # weights of every kind reach the fit
    rng = np.random.default_rng(5)
    w = rng.uniform(0.2, 2.0, f.shape[:2]).astype(F32)
    w[rng.random(w.shape) < 0.2] = 0
    assert np.abs(fit_flow_affine(f, weight=w) - R.fit_ref(f, "affine", w)).max() <= E2E_TOL
    assert np.abs(fit_flow_affine(f, weight=(w > 1).astype(np.uint8)) - R.fit_ref(f, "affine", (w > 1).astype(np.uint8))).max() \
        <= E2E_TOL
    cw = np.array([[1, 0, 2, 0.5], [0.25, 1, 0, 1], [1, 1, 3, 0], [0, 2, 1, 1]], F64)      # a float64 map, as the QC maps are
    assert np.abs(fit_flow_affine(f, weight=cw, cell_size=(32, 50)) - R.fit_ref(f, "affine", cw.astype(F32), (32, 50))).max() \
        <= E2E_TOL
    for shape, model in (((1, 64), "affine"), ((64, 1), "affine"), ((1, 1), "similarity")):
        with pytest.raises(ValueError, match="rank deficient"):
            fit_flow_affine(rotation_flow(shape), model)
    strip = rotation_flow((1, 64))
    assert np.abs(fit_flow_affine(strip, "similarity") - R.fit_ref(strip, "similarity")).max() <= 1e-9
    with pytest.raises(ValueError, match="rank deficient"):
        fit_flow_affine(f, weight=np.zeros(f.shape[:2], np.uint8))


def test_trim_follows_the_statements_rounds(ctx):
    clean = R.bumpy_flow()
    f = clean.copy()
    f[20:50, 40:90] += F32(25.0)
    keep = np.ones(f.shape[:2], np.uint8)
    keep[20:50, 40:90] = 0
    Tc, per_round, _ = FA.fit_from_moments(lambda p, c: tuple(m[0, 0] for m in R.moments_ref(f, None, None, p, c)[:2]),
                                           "affine", 2.0, 5)
    got, info = fit_flow_affine(f, trim=2.0, rounds=5, return_info=True)
    assert info.counts == per_round and info.counts[-1] == (97 * 161 - 1500, 0, 0, 1500)
    assert np.abs(got - FA._to_absolute(Tc, f.shape)).max() <= E2E_TOL
    assert np.abs(got - R.fit_ref(f, "affine", keep)).max() <= E2E_TOL
    assert fit_flow_affine(f, trim=2.0, rounds=1, return_info=True)[1].counts == per_round[:2]


def test_split_join_and_the_warp_positions(ctx):
    f = R.bumpy_flow()
    H, W = f.shape[:2]
    T, rest, info = split_flow(f, return_info=True)
    assert isinstance(rest, np.ndarray) and same_bits(rest, R.apply_ref(f, T))
    assert np.abs(T - fit_flow_affine(f)).max() == 0
    assert abs(info.residual_rms - R.weighted_rms(f, T)) <= 1e-6 and info.residual_rms < 0.35 < info.rms
    back = join_flow(T, rest)
    assert same_bits(back, R.apply_ref(rest, R.inverse(T)))
    assert np.abs(back.astype(F64) - f).max() <= 2.0 ** -23 * max(1.0, float(np.abs(f).max()))
    # a given matrix is used as it is
    T2 = np.array([[1.0, 0.01, -2.0], [-0.01, 1.0, 1.0]])
    t, r2, info2 = split_flow(f, T2, return_info=True)
    assert np.array_equal(t, T2) and same_bits(r2, R.apply_ref(f, T2)) and info2.model is None
    assert abs(info2.residual_rms - R.weighted_rms(f, T2)) <= 1e-6
    # Warper(flow=join(T, f')) samples where Warper(tmat=T, flow=f') does
    ys, xs = np.mgrid[0:H:7, 0:W:9].astype(F64)
    grid = np.stack([xs.ravel(), ys.ravel()], -1)
    a = transform_points(grid, back, "to_moving")
    b = transform_points(grid, rest, "to_moving", tmat=T)
    assert np.abs(a - b).max() <= 2.0 ** -23 * max(H, W)
    # DeviceArray in, DeviceArray out; a FlowGrid stands for its expansion
    d = ctx.asdevice(f)
    Td, rd = split_flow(d)
    assert isinstance(rd, DeviceArray) and np.array_equal(Td, T) and same_bits(rd.numpy(), rest)
    jd = join_flow(T, rd)
    assert isinstance(jd, DeviceArray) and same_bits(jd.numpy(), back)
    smooth = make_flow(65, 129)[0]
    nodes = np.ascontiguousarray(smooth[::8, ::8])
    grid_flow, dgrid = FlowGrid(nodes, 8, (65, 129)), FlowGrid(ctx.asdevice(nodes), 8, (65, 129))
    dense = grid_flow.expand()
    Tg = fit_flow_affine(dense, "similarity")
    assert np.array_equal(fit_flow_affine(grid_flow, "similarity"), Tg) and np.array_equal(fit_flow_affine(dgrid, "similarity"), Tg)
    tg, rg = split_flow(grid_flow, model="similarity")
    assert isinstance(rg, np.ndarray) and same_bits(rg, split_flow(dense, model="similarity")[1])
    assert isinstance(split_flow(dgrid)[1], DeviceArray) and isinstance(join_flow(Tg, dgrid), DeviceArray)
    assert same_bits(join_flow(Tg, grid_flow), join_flow(Tg, dense))
    assert np.array_equal(local_affine(grid_flow, 32).tmat, local_affine(dense, 32).tmat, equal_nan=True)


def test_local_affine_is_the_solve_of_the_cells_moments(ctx):
    f, rng = make_flow(96, 161, odd=True)
    w = make_weight("cells", 96, 161, rng, (32, 50))
    for weight in (None, w, make_weight("u8", 96, 161, rng, None)):
        exp_sums, exp_counts, _ = R.moments_ref(f, weight, (32, 50))
        for model in ("affine", "rigid"):
            exp = FA.affine_maps(exp_sums, exp_counts, (96, 161), (32, 50), model)
            got = local_affine(f, (32, 50), model, weight)
            assert np.array_equal(got.deficient, exp.deficient) and np.array_equal(got.used, exp.used)
            assert np.array_equal(got.cell_bounds, exp.cell_bounds)
            ok = ~exp.deficient
            assert np.abs(got.tmat[ok] - exp.tmat[ok]).max() <= 1e-9 and np.isnan(got.tmat[~ok]).all()
            for name in ("rotation_deg", "scale", "anisotropy", "shift_x", "shift_y", "rms"):
                assert np.allclose(getattr(got, name), getattr(exp, name), rtol=0, atol=1e-8, equal_nan=True), name
            assert got.summary()["cells"] == 12
    assert local_affine(f, (32, 50), weight=w).deficient.any()
    maps = local_affine(ctx.asdevice(f), 1000, "translation")
    assert maps.tmat.shape == (1, 1, 2, 3) and not maps.deficient.any()


def test_bad_arguments_are_refused_by_the_c_entries(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    f, _ = make_flow(H, W)
    d, out = ctx.asdevice(f), ctx.empty(f.shape, F32)
    w32 = ctx.asdevice(np.ones((H, W), F32))
    sums, counts = (C.c_double * 14)(), (C.c_longlong * 4)()
    prior = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    ok = dict(flow=d.ptr, H=H, W=W, weight=None, kind=0, ch=H, cw=W, prior=None, clip=0.0, sums=sums, counts=counts)
    mo = lambda **kw: ctx._run(ctx.lib.ma_flow_affine_moments, *dict(ok, **kw).values())     # noqa: E731
    mo()
    assert counts[0] == H * W
    mo(weight=w32.ptr, kind=1, prior=prior, clip=2.0)
    mo(ch=1 << 30, cw=1 << 30)                             # a cell larger than the image is the whole axis
    for kw in (dict(flow=None), dict(sums=None), dict(counts=None), dict(H=0), dict(W=0), dict(H=-1), dict(H=big),
               dict(W=big), dict(kind=-1), dict(kind=4), dict(kind=1), dict(kind=2), dict(kind=3), dict(ch=0), dict(cw=0),
               dict(ch=-3), dict(prior=prior, clip=0.0), dict(prior=prior, clip=-1.0), dict(prior=prior, clip=float("nan")),
               dict(prior=(C.c_double * 6)(1, 0, float("nan"), 0, 1, 0), clip=1.0),
               dict(prior=(C.c_double * 6)(1, 0, 0, 0, float("inf"), 0), clip=1.0), dict(flow=d.ptr + 4)):
        with pytest.raises(ValueError):
            mo(**kw)
    assert ctx.lib.ma_flow_affine_moments(None, *ok.values()) == _lib.MA_EINVAL
    a = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    oka = dict(flow=d.ptr, H=H, W=W, a=a, out=out.ptr)
    ap = lambda **kw: ctx._run(ctx.lib.ma_flow_affine_apply, *dict(oka, **kw).values())      # noqa: E731
    ap()
    for kw in (dict(flow=None), dict(a=None), dict(out=None), dict(H=0), dict(W=0), dict(H=big), dict(W=big),
               dict(a=(C.c_double * 6)(1, 0, 0, float("nan"), 1, 0)), dict(a=(C.c_double * 6)(1, 0, 0, 0, 1, float("-inf")))):
        with pytest.raises(ValueError):
            ap(**kw)
    assert ctx.lib.ma_flow_affine_apply(None, *oka.values()) == _lib.MA_EINVAL
    assert same_bits(d.numpy(), f) and same_bits(out.numpy(), R.apply_ref(f, a))     # refused calls wrote nothing


def test_entry_points_refuse_before_any_device_call(ctx, monkeypatch):
    f, _ = make_flow(20, 30)
    d = ctx.asdevice(f)
    w, w31 = ctx.asdevice(np.ones((20, 30), F32)), ctx.asdevice(np.ones((20, 31), F32))
    T = np.array([[1, 0, 0], [0, 1, 0]], F64)
    calls = []
    monkeypatch.setattr(type(ctx), "_run", lambda self, fn, *a: calls.append(fn))
    monkeypatch.setattr(type(ctx), "empty", lambda self, *a: calls.append("empty"))
    for kw in (dict(flow=w), dict(weight=w31), dict(weight=w31, cell_size=8), dict(cell_size=0), dict(prior=T),
               dict(clip=2.0), dict(prior=T, clip=0.0), dict(prior=T[:, :2], clip=1.0), dict(prior=T * np.nan, clip=1.0)):
        with pytest.raises(ValueError):
            ctx.flow_affine_moments(**dict(dict(flow=d), **kw))
    for kw in (dict(flow=w), dict(mat=np.eye(3)), dict(mat=np.full((2, 3), np.inf)), dict(out=w)):
        with pytest.raises(ValueError):
            ctx.flow_affine_apply(**dict(dict(flow=d, mat=T), **kw))
    for call in (lambda: fit_flow_affine(d, "homography"), lambda: fit_flow_affine(d, weight=w31),
                 lambda: fit_flow_affine(d, trim=0), lambda: split_flow(d, trim=-1.0), lambda: split_flow(d, np.eye(3)),
                 lambda: join_flow([[1, 2, 0], [2, 4, 0]], d), lambda: local_affine(d, 0), lambda: local_affine(w, 8)):
        with pytest.raises(ValueError):
            call()
    assert calls == []


def test_header_library_and_bindings_agree():
    import microaligner_amd
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_flow_affine_apply", "ma_flow_affine_moments"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_flowaffine.h but not exported"
        proto = re.search(r"\b" + n + r"\s*\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.FLOWAFFINE_SIGNATURES[n][1]), n
    assert sorted(_lib.FLOWAFFINE_SIGNATURES) == names
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES, _lib.FLOWCOMPOSE_SIGNATURES,
              _lib.FLOWINVERT_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.FLOWGRID_SIGNATURES, _lib.FLOWSMOOTH_SIGNATURES]
    assert not any(set(_lib.FLOWAFFINE_SIGNATURES) & set(t) for t in others)
    for name, value in re.findall(r"\b(MA_[A-Z0-9_]+)\s+(\d+)\b", text):
        assert getattr(_lib, name) == int(value), name
    assert {"fit_flow_affine", "split_flow", "join_flow", "local_affine"} <= set(microaligner_amd.__all__)
