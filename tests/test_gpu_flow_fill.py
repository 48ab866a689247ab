"""-m gpu: the push-pull fill of a flow on the device.  ma_fill_flow against the numpy float32 statement of
include/microaligner_flowfill.h (tests/_flow_fill_ref.py) bit for bit, with the three counts: every weight kind at shapes
that are odd at every level, single rows and columns and both sides of the kernels' tile edges; a hole crossed only near
the top of the pyramid; hard values; in place; the entry points; refused arguments; and the recipe with smooth_flow and
compress_flow."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_fill_ref as R  # noqa: E402
from microaligner_amd import FillInfo, FlowGrid, _lib, compress_flow, fill_flow, smooth_flow  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402
from test_gpu_flow_invert import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FLT_MAX = np.finfo(F32).max

# the issue's list, and the tile of the level-0 kernels (8 rows x 128 columns: 4 x 64 parents) +- 1, either way round; the
# tiles of the levels above are met by the larger shapes as they shrink
SHAPES = [(1, 1), (1, 2), (2, 1), (1, 300), (300, 1), (3, 5), (7, 5), (13, 64), (9, 700),
          (63, 127), (64, 128), (65, 129), (127, 63), (128, 64), (129, 65), (40, 255), (40, 256), (40, 257),
          (7, 127), (8, 128), (9, 129), (127, 7), (128, 8), (129, 9)]
CELLS = (16, 48)
KINDS = ("none", "f32", "u8", "cells")


def make_flow(H, W, seed=0, noise=0.3):
    rng = np.random.default_rng(1000 * H + W + seed)
    return (R.smooth_field(H, W) + rng.normal(0, noise, (H, W, 2))).astype(F32), rng


def make_weight(kind, H, W, rng):
    """(weight, cell_size) of a kind: about a third of the pixels (or cells) dropped and a block of 17 x 17 pixels (or the
    first cell) dropped entirely; the float32 kinds hold soft values in (0, 1) and values above 1, the uint8 kind values
    other than 1"""
    if kind == "none":
        return None, None
    if kind == "cells":
        gy, gx = -(-H // CELLS[0]), -(-W // CELLS[1])
        w = rng.uniform(0.5, 1.5, (gy, gx)).astype(F32)
        w[rng.random((gy, gx)) < 0.3] = 0
        w[0, 0] = 0
        return w, CELLS
    if kind == "f32":
        w = rng.uniform(0.25, 2.0, (H, W)).astype(F32)
        w[rng.random((H, W)) < 0.3] = 0
    else:
        w = (rng.random((H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
    w[H // 3:H // 3 + 17, W // 4:W // 4 + 17] = 0
    return w, None


def check(ctx, f, weight=None, cells=None):
    """one (flow, weight) against the statement: out of place, then in place; -> the counts"""
    exp, counts, L = R.fill_flow_ref(f, weight, cells)
    d = ctx.asdevice(f)
    dw = None if weight is None else ctx.asdevice(weight)
    out, info = ctx.fill_flow(d, dw, cells, return_info=True)
    assert out is not d and same_bits(out.numpy(), exp)
    assert isinstance(info, FillInfo) and tuple(info) == counts + (L,)
    assert same_bits(d.numpy(), f)
    got, info = ctx.fill_flow(d, dw, cells, return_info=True, out=d)
    assert got is d and same_bits(d.numpy(), exp) and tuple(info) == counts + (L,)
    return counts


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_numpy_statement_bit_for_bit(ctx, shape):
    f, rng = make_flow(*shape)
    f[rng.random(shape) < 0.02] = np.nan
    for kind in KINDS:
        weight, cells = make_weight(kind, *shape, rng)
        counts = check(ctx, f, weight, cells)
        assert counts[0] > 0 or shape[0] * shape[1] < 50
        if kind == "f32" and shape[0] * shape[1] > 1000:
            assert counts[1] > 0, "soft weights: blended pixels"


def test_a_larger_flow_with_a_hole_crossed_only_near_the_top(ctx):
    """(1031, 2049) with a 600 x 900 hole: 12 levels, entries with nothing kept up to level 8 (blocks of 256 x 256 pixels
    inside the hole), so the hole's middle is filled from level 9 and above"""
    H, W = 1031, 2049
    f, rng = make_flow(H, W)
    keep = np.ones((H, W), np.uint8)
    keep[200:800, 500:1400] = 0
    f[200:800, 500:1400] = np.nan
    counts = check(ctx, f, keep)
    assert counts == (600 * 900, 0, 0)
    soft = rng.uniform(0.0, 1.2, (H, W)).astype(F32)
    assert check(ctx, f, soft)[1] > 0


def hard_cases():
    f, rng = make_flow(45, 131, 3)
    vals = ((np.nan, 1.0), (np.inf, -np.inf), (-np.inf, np.nan), (FLT_MAX, -FLT_MAX), (2.0, np.nan), (-FLT_MAX, FLT_MAX),
            (1e-42, -1e-45), (FLT_MAX, FLT_MAX), (-FLT_MAX, 1e-45))
    for k in range(60):
        f[(5 + 11 * k) % 45, (6 + 37 * k) % 131] = vals[k % len(vals)]
    yield "non-finite, FLT_MAX and denormal components", f, None
    g, _ = make_flow(45, 131, 4)
    w = rng.uniform(0.1, 1.5, (45, 131)).astype(F32)
    for k in range(90):
        w[(3 + 7 * k) % 45, (2 + 29 * k) % 131] = (np.nan, -1.0, 0.0, np.inf, 1e30, 1e-40, -np.inf, -0.0, 3e38, 1e-45)[k % 10]
    yield "hard weights", g, w
    yield "hard weights and hard values", f, w
    big = (np.sign(g) * FLT_MAX * (0.5 + 0.5 * rng.random((45, 131, 2)))).astype(F32)
    yield "a field near FLT_MAX whose sums overflow", big, None
    yield "near FLT_MAX with soft weights", big, rng.uniform(0.0, 1.5, (45, 131)).astype(F32)
    yield "denormals", (rng.integers(-40, 40, (33, 70, 2)).astype(F64) * 1.4e-45).astype(F32), \
        (rng.random((33, 70)) * (rng.random((33, 70)) < 0.6)).astype(F32)
    yield "denormal weights only", g, np.full((45, 131), 1e-42, F32) * (rng.random((45, 131)) < 0.5)
    yield "all dropped by the weight", g, np.zeros((45, 131), np.uint8)
    yield "all dropped by the values", np.full((19, 70, 2), np.nan, F32), None
    corner = np.zeros((45, 131), np.uint8)
    corner[44, 130] = 3
    yield "one kept pixel in a corner", g, corner
    yield "one pixel, dropped", np.full((1, 1, 2), np.inf, F32), None
    yield "one pixel, soft", np.full((1, 1, 2), 3.0, F32), np.full((1, 1), 0.5, F32)


HARD = {name: (f, w) for name, f, w in hard_cases()}


@pytest.mark.parametrize("name", sorted(HARD))
def test_hard_values(ctx, name):
    f, w = HARD[name]
    H, W = f.shape[:2]
    counts = check(ctx, f, None if w is None else np.ascontiguousarray(w, w.dtype))
    if name.startswith("all dropped"):
        assert counts == (H * W, 0, H * W)
    if name == "one kept pixel in a corner":
        out = ctx.fill_flow(ctx.asdevice(f), ctx.asdevice(w)).numpy()
        assert counts == (H * W - 1, 0, 0) and same_bits(out, np.broadcast_to(f[44, 130], f.shape).copy())
    if name == "a field near FLT_MAX whose sums overflow":
        assert counts[0] == 0 and counts[2] == 0          # nothing dropped: every pixel is its own, whatever the sums did
    if name == "near FLT_MAX with soft weights":
        assert counts[2] > 0                              # the statement decides: overflowed sums reach blended pixels
    if name == "one pixel, soft":
        assert counts == (0, 1, 0)


def test_in_place_with_every_weight_kind_gives_the_same_bits(ctx):
    f, rng = make_flow(129, 257)
    f[40:90, 100:200] = np.nan
    for kind in KINDS:
        weight, cells = make_weight(kind, 129, 257, rng)
        check(ctx, f, weight, cells)              # out of place, then out=d
    other = ctx.empty(f.shape, F32)
    assert ctx.fill_flow(ctx.asdevice(f), out=other) is other and same_bits(other.numpy(), R.fill_flow_ref(f)[0])


# ---- entry points ----------------------------------------------------------------------------------------------------------
def test_entry_points_take_numpy_device_arrays_and_grids(ctx):
    H, W = 65, 129
    f, rng = make_flow(H, W)
    f[30:36, 50:70] = np.nan
    exp, counts, L = R.fill_flow_ref(f)
    out = fill_flow(f)
    assert isinstance(out, np.ndarray) and same_bits(out, exp)
    out, info = fill_flow(ctx.asdevice(f), return_info=True)
    assert isinstance(out, DeviceArray) and same_bits(out.numpy(), exp) and info == FillInfo(*counts, L) and info.levels == 8
    out, info = fill_flow(f, return_info=True)
    assert isinstance(out, np.ndarray) and same_bits(out, exp) and info == FillInfo(120, 0, 0, 8)
    # a mask on the host with the flow on the device, and the other way round
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
    expm = R.fill_flow_ref(f, mask)[0]
    assert same_bits(fill_flow(ctx.asdevice(f), weight=mask).numpy(), expm)
    assert same_bits(fill_flow(f, weight=ctx.asdevice(mask)), expm)
    soft = rng.uniform(0, 1.3, (H, W)).astype(F32)
    assert same_bits(fill_flow(f, soft), R.fill_flow_ref(f, soft)[0])
    # per-cell maps of any real dtype, as flow_qc gives them
    cellw = rng.random((-(-H // 16), -(-W // 48))) < 0.7
    expc = R.fill_flow_ref(f, cellw.astype(F32), (16, 48))[0]
    assert same_bits(fill_flow(f, weight=cellw, cell_size=(16, 48)), expc)
    assert same_bits(fill_flow(f, weight=cellw.astype(np.int64), cell_size=(16, 48)), expc)
    # a FlowGrid stands for its flow and gives the kind of array its nodes are
    nodes = np.ascontiguousarray(make_flow(H, W, noise=0.0)[0][::8, ::8])
    nodes[2:4, 5:9] = np.nan
    grid = FlowGrid(nodes, 8, (H, W))
    expg, countsg, _ = R.fill_flow_ref(grid.expand())
    out = fill_flow(grid)
    assert countsg[0] > 0 and isinstance(out, np.ndarray) and same_bits(out, expg)
    out = fill_flow(FlowGrid(ctx.asdevice(nodes), 8, (H, W)))
    assert isinstance(out, DeviceArray) and same_bits(out.numpy(), expg)


def test_the_c_entry_only_enqueues_without_counts_and_refuses_bad_arguments(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    f, _ = make_flow(H, W)
    f[10:20, 10:30] = np.nan
    d, out = ctx.asdevice(f), ctx.empty(f.shape, F32)
    w32, w8 = ctx.asdevice(np.ones((H, W), F32)), ctx.asdevice(np.ones((H, W), np.uint8))
    ok = dict(flow=d.ptr, H=H, W=W, weight=None, kind=0, ch=1, cw=1, out=out.ptr, counts=None)
    ff = lambda **kw: ctx._run(ctx.lib.ma_fill_flow, *dict(ok, **kw).values())     # noqa: E731
    ff()
    assert same_bits(out.numpy(), R.fill_flow_ref(f)[0])
    ff(weight=w32.ptr, kind=1)
    ff(weight=w8.ptr, kind=2, ch=0, cw=-5)            # the cell size is read for the cell kind only
    ff(weight=w32.ptr, kind=3, ch=1000, cw=1000)
    for kw in (dict(flow=None), dict(out=None), dict(H=0), dict(W=0), dict(H=-1), dict(H=big), dict(W=big), dict(kind=-1),
               dict(kind=4), dict(kind=1), dict(kind=2), dict(kind=3), dict(weight=w32.ptr, kind=3, ch=0, cw=4),
               dict(weight=w32.ptr, kind=3, ch=4, cw=0), dict(weight=out.ptr, kind=1), dict(weight=out.ptr, kind=3, ch=8, cw=8)):
        with pytest.raises(ValueError):
            ff(**kw)
    assert ctx.lib.ma_fill_flow(None, *ok.values()) == _lib.MA_EINVAL
    assert same_bits(d.numpy(), f)                                    # a refused call wrote nothing


def test_the_context_refuses_before_any_device_call(ctx, monkeypatch):
    f, _ = make_flow(20, 30)
    d = ctx.asdevice(f)
    w, w31 = ctx.asdevice(np.ones((20, 30), F32)), ctx.asdevice(np.ones((20, 31), F32))
    w16, d3, pair = ctx.asdevice(np.ones((20, 30), np.uint16)), ctx.asdevice(np.zeros((20, 30, 3), F32)), ctx.asdevice(f.copy())
    as_weight, cells32 = ctx.asdevice(np.ones((20, 30, 2), F32)), ctx.asdevice(np.ones((3, 2), F32))
    calls = []
    monkeypatch.setattr(type(ctx), "_run", lambda self, fn, *a: calls.append(fn))
    monkeypatch.setattr(type(ctx), "empty", lambda self, *a: calls.append("empty"))
    for kw in (dict(flow=w16), dict(flow=d3), dict(flow=w), dict(weight=w31), dict(weight=w16),
               dict(weight=cells32), dict(cell_size=5), dict(weight=w, cell_size=5), dict(out=w),
               dict(out=d3), dict(weight=as_weight), dict(weight=w, out=w)):
        with pytest.raises(ValueError):
            ctx.fill_flow(**dict(dict(flow=d), **kw))
    for kw in (dict(flow=f.astype(F64)), dict(flow=f[..., 0]), dict(weight=np.ones((20, 31), F32)),
               dict(weight=np.ones((3, 2), F32)), dict(cell_size=8)):
        with pytest.raises(ValueError):
            fill_flow(**dict(dict(flow=f), **kw))
    assert calls == []
    assert ctx.fill_flow(d, out=pair) is pair and len(calls) == 1


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_a_hole_wider_than_the_smoothing_reaches(ctx):
    """smooth_flow(sigma=6, where="blend") reaches 18 px: a 120 x 160 hole keeps unsupported pixels, and the grid of that flow
    has invalid pixels; fill_flow leaves none, kept pixels bit for bit, and compress_flow of the result has no invalid cell"""
    H, W = 256, 384
    f = R.smooth_field(H, W, scale=4.0)
    keep = np.ones((H, W), np.uint8)
    keep[60:180, 100:260] = 0
    holed = np.where(keep[..., None] > 0, f, F32(np.nan))
    smoothed, sinfo = smooth_flow(holed, 6.0, weight=keep, where="blend", return_info=True)
    assert sinfo.unsupported >= (120 - 36) * (160 - 36) and np.isnan(smoothed).any()
    _, err = compress_flow(smoothed, stride=8, cell_size=64, return_error=True)
    assert err.invalid.sum() > 0
    filled, info = fill_flow(holed, weight=keep, return_info=True)
    assert info == FillInfo(120 * 160, 0, 0, 9) and np.isfinite(filled).all()
    assert same_bits(filled[keep > 0], f[keep > 0])
    grid, err = compress_flow(filled, stride=8, cell_size=64, return_error=True)
    assert err.invalid.sum() == 0 and np.isfinite(grid.nodes).all()
    # within the range of the kept values, as the statement's CPU test derives
    slack = 8 * 9 * 2.0 ** -24 * np.abs(f).max()
    kept = f[keep > 0]
    assert np.all(filled.min((0, 1)) >= kept.min(0) - slack) and np.all(filled.max((0, 1)) <= kept.max(0) + slack)
