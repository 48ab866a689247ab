"""-m gpu: the weighted smoothing of a flow, the fold mask and the repair loop on the device.  ma_smooth_flow and
ma_flow_fold_mask against the numpy float32 statement of include/microaligner_flowsmooth.h (tests/_flow_smooth_ref.py) bit
for bit; the counts against flow_qc; the entry points; refused arguments; the plumbing of the new header."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_smooth_ref as R  # noqa: E402
from microaligner_amd import FlowGrid, _lib, flow_qc, fold_mask, repair_flow, smooth_flow  # noqa: E402
from microaligner_amd.device import DeviceArray, gaussian_taps  # noqa: E402
from test_gpu_flow_invert import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowsmooth.h")

# the shape list of the composition's and the inverse's tests, and the smoothing tile (64 lines x 128 outputs, either way
# round) +- 1
SHAPES = [(1, 1), (1, 300), (300, 1), (40, 255), (40, 256), (40, 257), (13, 64), (9, 700), (7, 5),
          (63, 127), (64, 128), (65, 129), (127, 63), (128, 64), (129, 65)]
CELLS = (16, 48)


def make_flow(H, W, seed=0, noise=0.3):
    """a smooth flow plus pixel noise (which folds here and there); noise=0: smooth, nothing folds"""
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    f = np.stack([3 * np.sin(x / 17) + 2 * np.cos(y / 23), 2.5 * np.cos(x / 13 + y / 31)], -1)
    return (f + rng.normal(0, noise, (H, W, 2))).astype(F32), rng


def make_weight(kind, H, W, rng):
    """(weight, cell_size) of a kind; about a third of the pixels (or cells) dropped"""
    if kind == "none":
        return None, None
    if kind == "f32":
        w = rng.uniform(0.25, 2.0, (H, W)).astype(F32)
        w[rng.random((H, W)) < 0.3] = 0
        return w, None
    if kind == "u8":
        w = (rng.random((H, W)) < 0.7).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
        w[H // 3:H // 3 + 9, W // 4:W // 4 + 40] = 0
        return w, None
    gy, gx = -(-H // CELLS[0]), -(-W // CELLS[1])
    w = rng.uniform(0.5, 1.5, (gy, gx)).astype(F32)
    w[rng.random((gy, gx)) < 0.3] = 0
    return w, CELLS


def check(ctx, f, taps, weight, cells, mode, min_support, out=None):
    exp, exp_un = R.smooth_flow_ref(f, taps, weight, cells, mode, min_support)
    d = ctx.asdevice(f) if out is None else out
    got, info = ctx.smooth_flow(d, taps, None if weight is None else ctx.asdevice(weight), cells, mode, min_support,
                                return_info=True, out=out)
    assert same_bits(got.numpy(), exp)
    assert info.unsupported == exp_un
    return exp_un


def taps_of(r, rng=None):
    """Gaussian taps of radius r; with rng, arbitrary non-negative ones (zeros among them)"""
    if rng is None:
        sigma = r / 3.0
        return gaussian_taps(sigma, (r - 0.5) / sigma)      # ceil(r - 0.5) = r whatever the rounding of the product
    t = rng.uniform(0, 1, r + 1).astype(F32)
    t[1::3] = 0
    t[0] = max(t[0], F32(0.01))
    return t


@pytest.mark.parametrize("r", [1, 2, 7, 64, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_numpy_statement_bit_for_bit(ctx, shape, r):
    """every weight kind x both modes x min_support 0 and 1e-3; images smaller than r are among the shapes"""
    f, rng = make_flow(*shape)
    taps = taps_of(r)
    assert len(taps) == r + 1
    for kind in ("none", "f32", "u8", "cells"):
        weight, cells = make_weight(kind, *shape, rng)
        for mode in ("all", "blend"):
            for min_support in (0.0, 1e-3):
                check(ctx, f, taps, weight, cells, mode, min_support)


@pytest.mark.parametrize("r", [3, 21, 100])
def test_arbitrary_taps_and_a_centre_only_kernel(ctx, r):
    f, rng = make_flow(70, 200, r)
    weight, _ = make_weight("u8", 70, 200, rng)
    check(ctx, f, taps_of(r, rng), weight, None, "blend", 0.0)
    only = np.zeros(r + 1, F32)
    only[0] = 0.5
    assert check(ctx, f, only, weight, None, "all", 0.0) == int((weight == 0).sum())


def test_a_large_flow(ctx):
    """(2049, 1031): many blocks either way, 64-bit offsets exercised by nothing smaller; r <= 21 keeps the statement quick"""
    f, rng = make_flow(2049, 1031)
    keep = np.ones((2049, 1031), np.uint8)
    for _ in range(40):
        y0, x0 = int(rng.integers(0, 2049)), int(rng.integers(0, 1031))
        keep[y0:y0 + int(rng.integers(1, 60)), x0:x0 + int(rng.integers(1, 60))] = 0
    assert check(ctx, f, gaussian_taps(7.0), keep, None, "blend", 0.0) > 0
    check(ctx, f, gaussian_taps(2.0), None, None, "all", 0.0)


def odd_values(f, rng):
    H, W = f.shape[:2]
    vals = ((np.nan, 1.0), (np.inf, -np.inf), (-np.inf, np.nan), (1e30, -1e30), (2.0, np.nan), (-1e30, 3e38), (1e-42, -1e-45))
    for k, v in enumerate(vals):
        f[(5 + 11 * k) % H, (6 + 37 * k) % W] = v
    return f


@pytest.mark.parametrize("shape", [(67, 301), (1, 1), (130, 64), (5, 40)])
@pytest.mark.parametrize("r", [2, 18, 128])
def test_non_finite_and_extreme_flows_and_weights(ctx, shape, r):
    """NaN, +-Inf, +-1e30 and denormal pixels; weights that are NaN, negative, 0, Inf, 1e30 or denormal.  The products
    overflow and the sums meet Inf - Inf: the kernels must give IEEE's answers where the statement does."""
    f, rng = make_flow(*shape)
    f = odd_values(f, rng)
    H, W = shape
    w = rng.uniform(0.5, 1.5, shape).astype(F32)
    for k, v in enumerate((np.nan, -1.0, 0.0, np.inf, 1e30, 1e-40, -np.inf, -0.0, 3e38)):
        w[(3 + 7 * k) % H, (2 + 29 * k) % W] = v
    taps = taps_of(r)
    for mode in ("all", "blend"):
        check(ctx, f, taps, None, None, mode, 0.0)
        check(ctx, f, taps, w, None, mode, 0.0)
        check(ctx, f, taps, w, None, mode, 1e-3)
    cw = np.resize(np.array([1.0, np.nan, 0.5, -2.0, np.inf, 0.0, 1e-40, 2.0, 1.0], F32), (-(-H // 16), -(-W // 200)))
    check(ctx, f, taps, cw, (16, 200), "blend", 0.0)


def test_out_may_be_the_flow(ctx):
    f, rng = make_flow(150, 333)
    weight, _ = make_weight("u8", 150, 333, rng)
    for mode in ("blend", "all"):
        d = ctx.asdevice(f.copy())
        check(ctx, f, gaussian_taps(5.0), weight, None, mode, 0.0, out=d)


# ---- fold mask -----------------------------------------------------------------------------------------------------------
def folding_flow(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    return np.stack([12 * np.sin(x / 9), 4 * np.cos(y / 5)], -1).astype(F32)


def mask_cases():
    yield "repair", R.repair_case()
    for shape in ((1, 1), (1, 300), (300, 1), (31, 63), (32, 64), (33, 65), (70, 300)):   # the mask tile is 32 x 64
        f = folding_flow(*shape)
        if shape[0] > 8 and shape[1] > 40:
            f = odd_values(f, None)
        yield str(shape), f
    f, _ = make_flow(40, 257, noise=0.0)
    yield "smooth", f


MASKS = dict(mask_cases())


@pytest.mark.parametrize("margin", [0, 1, 4, 32])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_fold_mask_equals_the_statement_and_flow_qc(ctx, name, margin):
    f = MASKS[name]
    exp_keep, exp_counts = R.fold_mask_ref(f, margin)
    keep, info = ctx.fold_mask(ctx.asdevice(f), margin, return_info=True)
    assert keep.dtype == np.uint8 and np.array_equal(keep.numpy(), exp_keep)
    assert tuple(info) == exp_counts
    qc = flow_qc(f, cell_size=64)
    assert info.folded == int(qc.folded.sum()) and info.invalid == int(qc.invalid.sum())
    assert np.array_equal(ctx.fold_mask(ctx.asdevice(f), margin).numpy(), exp_keep)      # the call that only enqueues
    if name == "repair":
        assert (info.folded, info.invalid) == (105, 1768)
    if name == "smooth":
        assert tuple(info) == (0, 0, 0)


# ---- repair ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma, margin, most", [(6.0, 4, 3), (4.0, 2, 4)])
def test_repair_flow_follows_the_statements_loop_round_by_round(ctx, sigma, margin, most):
    f = R.repair_case()
    exp, exp_rounds, exp_conv, steps = R.repair_flow_ref(f, sigma, margin)
    assert exp_conv and len(exp_rounds) <= most
    taps = gaussian_taps(sigma)
    cur = ctx.asdevice(f)
    for k, step in enumerate(steps):                       # the loop by hand: every round's flow
        keep, m = ctx.fold_mask(cur, margin, return_info=True)
        cur, s = ctx.smooth_flow(cur, taps, keep, None, "blend", 0.0, return_info=True)
        assert (m.folded, m.invalid, m.dropped, s.unsupported) == exp_rounds[k]
        assert same_bits(cur.numpy(), step)
    got, info = repair_flow(f, sigma, margin, return_info=True)
    assert isinstance(got, np.ndarray) and same_bits(got, exp)
    assert info.rounds == exp_rounds and info.converged
    qc = flow_qc(got, cell_size=32)
    assert int(qc.folded.sum()) == 0 and int(qc.invalid.sum()) == 0 and float(qc.jac_min.min()) > 0
    assert np.isfinite(got).all()


def test_repair_flow_reports_a_stall_and_leaves_a_clean_flow_alone(ctx):
    f = R.repair_case()
    exp, exp_rounds, exp_conv, _ = R.repair_flow_ref(f, 3.0, 2, 3)
    got, info = repair_flow(ctx.asdevice(f), 3.0, 2, max_rounds=3, return_info=True)
    assert isinstance(got, DeviceArray) and same_bits(got.numpy(), exp)
    assert not info.converged and not exp_conv and info.rounds == exp_rounds and len(info.rounds) == 3
    clean, _ = make_flow(50, 70, noise=0.0)
    d = ctx.asdevice(clean)
    got, info = repair_flow(d, return_info=True)
    assert got is not d and same_bits(got.numpy(), clean) and info.rounds == [] and info.converged
    assert same_bits(repair_flow(clean), clean)


# ---- entry points ----------------------------------------------------------------------------------------------------------
def test_entry_points_take_numpy_device_arrays_and_grids(ctx):
    H, W = 65, 129
    f, rng = make_flow(H, W)
    f[30:36, 50:70] = np.nan
    taps = R.gaussian_taps(2.0)
    exp, exp_un = R.smooth_flow_ref(f, taps)
    out = smooth_flow(f, 2.0)
    assert isinstance(out, np.ndarray) and same_bits(out, exp)
    out, info = smooth_flow(ctx.asdevice(f), 2.0, return_info=True)
    assert isinstance(out, DeviceArray) and same_bits(out.numpy(), exp) and info.unsupported == exp_un
    # truncate and min_support reach the kernel
    exp2, un2 = R.smooth_flow_ref(f, R.gaussian_taps(2.0, 1.5), None, None, "all", 0.5)
    out, info = smooth_flow(f, 2.0, truncate=1.5, min_support=0.5, return_info=True)
    assert same_bits(out, exp2) and info.unsupported == un2 > 0
    # a mask on the host with the flow on the device, and the other way round
    keep, kinfo = fold_mask(f, 3, return_info=True)
    exp_keep, exp_counts = R.fold_mask_ref(f, 3)
    assert isinstance(keep, np.ndarray) and np.array_equal(keep, exp_keep) and tuple(kinfo) == exp_counts
    dkeep = fold_mask(ctx.asdevice(f), 3)
    assert isinstance(dkeep, DeviceArray) and np.array_equal(dkeep.numpy(), exp_keep)
    expb, _ = R.smooth_flow_ref(f, taps, exp_keep, None, "blend")
    assert same_bits(smooth_flow(ctx.asdevice(f), 2.0, weight=keep, where="blend").numpy(), expb)
    assert same_bits(smooth_flow(f, 2.0, weight=dkeep, where="blend"), expb)
    # per-cell maps as flow_qc gives them: int64 / bool maps of (gy, gx) with the cell size
    qc = flow_qc(f, cell_size=(16, 48))
    cellw = (qc.invalid == 0)
    expc, _ = R.smooth_flow_ref(f, taps, cellw.astype(F32), (16, 48), "blend")
    assert same_bits(smooth_flow(f, 2.0, weight=cellw, cell_size=(16, 48), where="blend"), expc)
    assert same_bits(smooth_flow(f, 2.0, weight=ctx.asdevice(cellw.astype(F32)), cell_size=(16, 48), where="blend"), expc)
    # a FlowGrid stands for its flow and gives the kind of array its nodes are
    clean, _ = make_flow(H, W, noise=0.0)
    nodes = np.ascontiguousarray(clean[::8, ::8])
    grid = FlowGrid(nodes, 8, (H, W))
    dense = grid.expand()
    expg, _ = R.smooth_flow_ref(dense, taps)
    out = smooth_flow(grid, 2.0)
    assert isinstance(out, np.ndarray) and same_bits(out, expg)
    dgrid = FlowGrid(ctx.asdevice(nodes), 8, (H, W))
    out = smooth_flow(dgrid, 2.0)
    assert isinstance(out, DeviceArray) and same_bits(out.numpy(), expg)
    assert isinstance(fold_mask(grid), np.ndarray) and isinstance(fold_mask(dgrid), DeviceArray)
    assert isinstance(repair_flow(grid), np.ndarray) and isinstance(repair_flow(dgrid), DeviceArray)
    assert same_bits(repair_flow(grid), dense)


# ---- refused arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_c_entries(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    f, rng = make_flow(H, W)
    d, out = ctx.asdevice(f), ctx.empty(f.shape, F32)
    w32, w8 = ctx.asdevice(np.ones((H, W), F32)), ctx.asdevice(np.ones((H, W), np.uint8))
    taps = (C.c_float * 4)(0.4, 0.2, 0.1, 0.0)

    def bad_taps(*v):
        return (C.c_float * len(v))(*v)
    ok = dict(flow=d.ptr, H=H, W=W, taps=taps, r=3, weight=None, kind=0, ch=1, cw=1, mode=0, ms=0.0, out=out.ptr, un=None)
    sm = lambda **kw: ctx._run(ctx.lib.ma_smooth_flow, *dict(ok, **kw).values())     # noqa: E731
    sm()
    sm(weight=w32.ptr, kind=1, mode=1)
    sm(weight=w8.ptr, kind=2, ch=0, cw=-5)            # the cell size is read for the cell kind only
    sm(weight=w32.ptr, kind=3, ch=1000, cw=1000)
    for kw in (dict(flow=None), dict(taps=None), dict(out=None), dict(H=0), dict(W=0), dict(H=-1), dict(H=big),
               dict(W=big), dict(r=0), dict(r=-1), dict(r=129), dict(taps=bad_taps(0.0, 0.2, 0.1, 0.0)),
               dict(taps=bad_taps(0.4, -0.2, 0.1, 0.0)), dict(taps=bad_taps(0.4, 0.2, float("nan"), 0.0)),
               dict(taps=bad_taps(0.4, 0.2, 0.1, float("inf"))), dict(taps=bad_taps(float("nan"), 0.2, 0.1, 0.0)),
               dict(kind=-1), dict(kind=4), dict(kind=1), dict(kind=2), dict(kind=3), dict(mode=-1), dict(mode=2),
               dict(weight=w32.ptr, kind=3, ch=0, cw=4), dict(weight=w32.ptr, kind=3, ch=4, cw=0),
               dict(weight=w32.ptr, kind=3, ch=-1, cw=4), dict(ms=-1.0), dict(ms=float("nan")), dict(ms=float("inf")),
               dict(weight=out.ptr, kind=1)):
        with pytest.raises(ValueError):
            sm(**kw)
    assert ctx.lib.ma_smooth_flow(None, *ok.values()) == _lib.MA_EINVAL
    assert ctx.lib.ma_smooth_flow(ctx.handle, *dict(ok, r=200).values()) == _lib.MA_EINVAL

    keep = ctx.empty((H, W), np.uint8)
    okm = dict(flow=d.ptr, H=H, W=W, margin=2, keep=keep.ptr, counts=None)
    fm = lambda **kw: ctx._run(ctx.lib.ma_flow_fold_mask, *dict(okm, **kw).values())   # noqa: E731
    fm()
    for kw in (dict(flow=None), dict(keep=None), dict(H=0), dict(W=0), dict(H=big), dict(W=big), dict(margin=-1),
               dict(margin=33)):
        with pytest.raises(ValueError):
            fm(**kw)
    assert ctx.lib.ma_flow_fold_mask(None, *okm.values()) == _lib.MA_EINVAL
    assert ctx.lib.ma_flow_fold_mask(ctx.handle, *dict(okm, margin=64).values()) == _lib.MA_EINVAL
    assert same_bits(d.numpy(), f)                                    # a refused call wrote nothing


def test_entry_points_refuse_before_any_device_call(ctx, monkeypatch):
    """every refused argument raises ValueError with zero device calls: the context's own entry points count them"""
    f, _ = make_flow(20, 30)
    d = ctx.asdevice(f)
    w, w31 = ctx.asdevice(np.ones((20, 30), F32)), ctx.asdevice(np.ones((20, 31), F32))
    calls = []
    monkeypatch.setattr(type(ctx), "_run", lambda self, fn, *a: calls.append(fn))
    monkeypatch.setattr(type(ctx), "empty", lambda self, *a: calls.append("empty"))
    taps = gaussian_taps(2.0)
    for kw in (dict(taps=taps.astype(F64)), dict(taps=np.zeros(2, F32)), dict(taps=np.ones(130, F32)), dict(taps=taps[:1]),
               dict(taps=-taps), dict(taps=list(taps)), dict(where="some"), dict(min_support=-1.0),
               dict(min_support=float("nan")), dict(weight=w31), dict(cell_size=5),
               dict(weight=w, cell_size=5), dict(flow=w), dict(out=w)):
        with pytest.raises(ValueError):
            ctx.smooth_flow(**dict(dict(flow=d, taps=taps), **kw))
    for kw in (dict(margin=33), dict(margin=-1), dict(margin=1.5), dict(flow=w)):
        with pytest.raises(ValueError):
            ctx.fold_mask(**dict(dict(flow=d), **kw))
    assert calls == []


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    import microaligner_amd
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_flow_fold_mask", "ma_smooth_flow"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_flowsmooth.h but not exported"
        proto = re.search(r"\b" + n + r"\s*\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.FLOWSMOOTH_SIGNATURES[n][1]), n
    assert sorted(_lib.FLOWSMOOTH_SIGNATURES) == names
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES, _lib.FLOWCOMPOSE_SIGNATURES,
              _lib.FLOWINVERT_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.FLOWGRID_SIGNATURES]
    assert not any(set(_lib.FLOWSMOOTH_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_hip.h"' in open(HEADER).read()
    for name, value in re.findall(r"\b(MA_[A-Z0-9_]+)\s*=?\s+(\d+)\b", text):
        assert getattr(_lib, name) == int(value), name
    assert {"smooth_flow", "fold_mask", "repair_flow"} <= set(microaligner_amd.__all__)


def test_the_source_hash_is_the_parents(tmp_path, monkeypatch):
    """build.source_hash() reads the files and flags it read before this source existed: the library's hash is the
    tree's, and the hash taken with the new source and its headers struck from the build's lists -- what the parent
    commit computes from the same files -- is the same, as it is after an edit of the new source."""
    from microaligner_amd import build
    before = build.source_hash()
    assert _lib.source_hash() == before
    assert "flow_smooth.hip" in build.SOURCES and "microaligner_flowsmooth.h" not in " ".join(build.HEADERS)
    own = [os.path.basename(h) for h in build.SOURCE_HEADERS["flow_smooth.hip"]]
    assert own == ["microaligner_flowsmooth.h", "cell_grid.h", "flow_jacobian.h", "window_fir.h", "weight_map.h",
                   "call_counts.h"]
    assert "flow_jacobian.h" in [os.path.basename(h) for h in build.SOURCE_HEADERS["qc.hip"]]
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "flow_smooth.hip"])
    monkeypatch.setattr(build, "SOURCE_HEADERS", {k: v for k, v in build.SOURCE_HEADERS.items() if k != "flow_smooth.hip"})
    assert build.source_hash() == before
    monkeypatch.undo()
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc)
    headers = [str((csrc if os.path.samefile(os.path.dirname(h), build.CSRC) else tmp_path) / os.path.basename(h))
               for h in build.HEADERS]
    shutil.copy(os.path.join(ROOT, "include", "microaligner_hip.h"), tmp_path / "microaligner_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADERS", headers)
    assert build.source_hash() == before
    for name in ("flow_smooth.hip", "flow_jacobian.h", "window_fir.h", "qc.hip"):
        with open(csrc / name, "a") as fh:
            fh.write("\n// edited\n")
    assert build.source_hash() == before
    with open(csrc / "remap.hip", "a") as fh:
        fh.write("\n// edited\n")
    assert build.source_hash() != before
