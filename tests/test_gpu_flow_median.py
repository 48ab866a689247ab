"""-m gpu: the median filter of a flow and its outlier mask on the device.  ma_median_flow -- the generic kernel and the
register kernels of radius 1 to 3 -- against the numpy statement of include/microaligner_flowmedian.h
(tests/_flow_median_ref.py) bit for bit, with keep and the three counts; hard values; the effect on a spiked flow with a
bound derived from the inputs; the recipe with fold_mask and smooth_flow; the entry points; refused arguments; the
plumbing of the new header."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_median_ref as R  # noqa: E402
import _flow_smooth_ref as S  # noqa: E402
from microaligner_amd import FlowGrid, MedianInfo, _lib, fold_mask, median_flow, outlier_mask, smooth_flow  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402
from test_gpu_flow_invert import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FLT_MAX = np.finfo(F32).max
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowmedian.h")

# the shape list of the smoothing's tests, and the median's tile (32 rows x 64 columns) +- 1, either way round
SHAPES = [(1, 1), (1, 300), (300, 1), (7, 5), (13, 64), (9, 700), (40, 255), (40, 256), (40, 257),
          (31, 63), (32, 64), (33, 65), (63, 31), (64, 32), (65, 33)]
RADII = [1, 2, 3, 4, 7]
CELLS = (16, 48)
KINDS = ("none", "f32", "u8", "cells")


def make_flow(H, W, seed=0, noise=0.3):
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    f = np.stack([3 * np.sin(x / 17) + 2 * np.cos(y / 23), 2.5 * np.cos(x / 13 + y / 31)], -1)
    return (f + rng.normal(0, noise, (H, W, 2))).astype(F32), rng


def make_weight(kind, H, W, rng):
    """(weight, cell_size) of a kind: about a third of the pixels (or cells) dropped, and a block of 17 x 17 pixels (or the
    first cell) dropped entirely, so that whole windows of every radius are"""
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


def check(ctx, f, r, weight=None, cells=None, modes=("all", "outliers"), threshs=(0.0, 0.5, np.inf)):
    """every mode x thresh x kernel of one (flow, radius, weight) against the statement; the medians are computed once"""
    m, part, n = R.window_median(f, r, weight, cells)
    d = ctx.asdevice(f)
    dw = None if weight is None else ctx.asdevice(weight)
    counts = None
    for mode in modes:
        for thresh in threshs:
            exp, exp_keep, counts = R.finish(f, m, part, n, mode, thresh)
            for generic in ((False, True) if r <= 3 else (False,)):
                out, keep, info = ctx.median_flow(d, r, dw, cells, mode, thresh, return_info=True, keep=True, generic=generic)
                assert same_bits(out.numpy(), exp), (mode, thresh, generic)
                assert keep.dtype == np.uint8 and np.array_equal(keep.numpy(), exp_keep), (mode, thresh, generic)
                assert isinstance(info, MedianInfo) and tuple(info) == counts, (mode, thresh, generic)
    return counts


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_numpy_statement_bit_for_bit(ctx, shape, r):
    """every weight kind x both modes x thresh 0, 0.5 and +Inf; the register kernels and the generic one at r <= 3; images
    smaller than the window are among the shapes"""
    f, rng = make_flow(*shape)
    for kind in KINDS:
        weight, cells = make_weight(kind, *shape, rng)
        counts = check(ctx, f, r, weight, cells)
        if kind == "none":
            assert counts[1:] == (0, 0)
        elif shape in ((40, 257), (1, 300), (300, 1), (1, 1)):
            assert counts[2] > 0, "a whole window dropped: unsupported pixels"


def test_a_large_flow(ctx):
    """(1031, 2049): many blocks either way"""
    f, rng = make_flow(1031, 2049)
    keep = (rng.random((1031, 2049)) < 0.8).astype(np.uint8)
    for r in (2, 3):
        check(ctx, f, r, keep, None, ("outliers",), (0.5,))
    check(ctx, f, 1, None, None, ("all",), (np.inf,))


def hard_flows():
    f, _ = make_flow(45, 131, 3)
    vals = ((np.nan, 1.0), (np.inf, -np.inf), (-np.inf, np.nan), (FLT_MAX, -FLT_MAX), (2.0, np.nan), (-FLT_MAX, FLT_MAX),
            (1e-42, -1e-45), (FLT_MAX, FLT_MAX), (-FLT_MAX, 1e-45))
    for k in range(60):
        f[(5 + 11 * k) % 45, (6 + 37 * k) % 131] = vals[k % len(vals)]
    yield "non-finite and FLT_MAX", f
    rng = np.random.default_rng(5)
    yield "denormals", (rng.integers(-40, 40, (33, 70, 2)).astype(F64) * 1.4e-45).astype(F32)
    q = np.array([-1.0, -0.0, 0.0, 1.0, 2.0], F32)
    yield "quantised", q[rng.integers(0, 5, (37, 66, 2))]
    yield "signed zeros", q[rng.integers(1, 3, (20, 65, 2))]
    c = np.empty((33, 65, 2), F32)
    c[...] = (3.25, -1234.5)
    yield "constant", c
    yield "even windows", make_flow(2, 2, 1)[0]         # n = 4 in every window of radius >= 1
    yield "one row of two", make_flow(1, 2, 2)[0]


HARD = dict(hard_flows())


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("name", sorted(HARD))
def test_hard_values(ctx, name, r):
    f = HARD[name]
    H, W = f.shape[:2]
    counts = check(ctx, f, r)
    if name == "constant":
        assert counts == (0, 0, 0)
        assert same_bits(ctx.median_flow(ctx.asdevice(f), r, where="outliers", thresh=0.0).numpy(), f)
    if name == "non-finite and FLT_MAX":
        assert counts[1] > 0
    rng = np.random.default_rng(r)
    mask = (rng.random((H, W)) < 0.5).astype(np.uint8)          # even and odd counts of every size
    check(ctx, f, r, mask, None, ("outliers",), (0.5,))
    w = rng.uniform(0.5, 1.5, (H, W)).astype(F32)
    for k, v in enumerate((np.nan, -1.0, 0.0, np.inf, 1e30, 1e-40, -np.inf, -0.0, 3e38)):
        w[(3 + 7 * k) % H, (2 + 29 * k) % W] = v
    check(ctx, f, r, w, None, ("all",), (0.5,))


@pytest.mark.parametrize("r", [1, 2, 3])
def test_register_kernels_give_the_generic_kernels_bits(ctx, r):
    for name in sorted(HARD):
        f = HARD[name]
        rng = np.random.default_rng(r)
        w = ctx.asdevice((rng.random(f.shape[:2]) < 0.6).astype(np.uint8))
        d = ctx.asdevice(f)
        for weight in (None, w):
            a = ctx.median_flow(d, r, weight, None, "outliers", 0.25, return_info=True, keep=True)
            b = ctx.median_flow(d, r, weight, None, "outliers", 0.25, return_info=True, keep=True, generic=True)
            assert same_bits(a[0].numpy(), b[0].numpy()) and np.array_equal(a[1].numpy(), b[1].numpy()) and a[2] == b[2]


# ---- effect ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [2, 3])
def test_spikes_return_to_the_clean_flow_and_nothing_else_moves(ctx, r):
    """Fewer spikes than half of every window (asserted from the spike mask): the median of a window then lies between
    the smallest and the largest clean value of the window, which are within r (Lx + Ly) of the clean value at its
    centre.  So with thresh >= r (Lx + Ly) no clean pixel is an outlier, and every spike (20 px) is."""
    clean, spiked, spikes, Lx, Ly = R.spiked_flow()
    cnt, size = R.window_count(spikes, r)
    assert spikes.sum() > 50 and np.all(2 * cnt < size)
    bound = r * (Lx + Ly)
    thresh = float(F32(1.01 * bound))
    assert 20 - bound > thresh
    out, info = median_flow(spiked, r, where="outliers", thresh=thresh, return_info=True)
    assert np.abs(out.astype(F64) - clean)[spikes].max() <= bound
    assert same_bits(out[~spikes], spiked[~spikes])
    assert info == MedianInfo(int(spikes.sum()), 0, 0)
    keep = outlier_mask(spiked, r, thresh)
    assert np.array_equal(keep == 0, spikes)


def test_the_recipe_with_fold_mask_and_smooth_flow(ctx):
    """keep = fold_mask(flow, 2); keep = outlier_mask(flow, 2, 1.0, weight=keep); smooth_flow(flow, 4.0, weight=keep,
    where="blend"): equal to the statements chained, and it finds the spikes that do not fold"""
    clean, flow, spikes, Lx, Ly = R.spiked_flow(amp=1.6, scale=4.0, seed=1)
    assert 1.6 - 2 * (Lx + Ly) > 1.0
    flow[40:44, 60:70, 0] += np.linspace(0, -30, 10, dtype=F32)          # and a patch that folds
    keep1 = fold_mask(flow, margin=2)
    keep2 = outlier_mask(flow, radius=2, thresh=1.0, weight=keep1)
    out = smooth_flow(flow, 4.0, weight=keep2, where="blend")
    exp1, counts1 = S.fold_mask_ref(flow, 2)
    exp2 = R.median_flow_ref(flow, 2, exp1, None, "all", 1.0)[1]
    exp, _ = S.smooth_flow_ref(flow, S.gaussian_taps(4.0), exp2, None, "blend")
    assert np.array_equal(keep1, exp1) and np.array_equal(keep2, exp2) and same_bits(out, exp)
    assert counts1[0] > 0 and np.all(keep2 <= keep1)                      # a subset of the fold mask's keep
    assert keep1[spikes].sum() > 0.8 * spikes.sum()                       # the fold mask keeps most spikes ...
    assert not keep2[spikes].any()                                        # ... the outlier mask none
    far = keep1.astype(bool)
    assert np.abs(out - clean)[far].max() < 0.5 < np.abs(flow - clean)[far].max()


# ---- entry points ----------------------------------------------------------------------------------------------------------
def test_entry_points_take_numpy_device_arrays_and_grids(ctx):
    H, W = 65, 129
    f, rng = make_flow(H, W)
    f[30:36, 50:70] = np.nan
    exp, exp_keep, counts = R.median_flow_ref(f, 2)
    out = median_flow(f)
    assert isinstance(out, np.ndarray) and same_bits(out, exp)
    out, info = median_flow(ctx.asdevice(f), return_info=True)
    assert isinstance(out, DeviceArray) and same_bits(out.numpy(), exp) and tuple(info) == counts
    exp3, keep3, counts3 = R.median_flow_ref(f, 3, None, None, "outliers", 0.4)
    out, info = median_flow(f, 3, where="outliers", thresh=0.4, return_info=True)
    assert same_bits(out, exp3) and tuple(info) == counts3
    keep, info = outlier_mask(f, 3, 0.4, return_info=True)
    assert isinstance(keep, np.ndarray) and keep.dtype == np.uint8 and np.array_equal(keep, keep3) and tuple(info) == counts3
    dkeep = outlier_mask(ctx.asdevice(f), 3, 0.4)
    assert isinstance(dkeep, DeviceArray) and np.array_equal(dkeep.numpy(), keep3)
    # a mask on the host with the flow on the device, and the other way round
    mask = (rng.random((H, W)) < 0.7).astype(np.uint8)
    expm = R.median_flow_ref(f, 2, mask)[0]
    assert same_bits(median_flow(ctx.asdevice(f), weight=mask).numpy(), expm)
    assert same_bits(median_flow(f, weight=ctx.asdevice(mask)), expm)
    # per-cell maps of any real dtype, as flow_qc gives them
    cellw = rng.random((-(-H // 16), -(-W // 48))) < 0.7
    expc, keepc, _ = R.median_flow_ref(f, 2, cellw.astype(F32), (16, 48), "all", 1.0)
    assert same_bits(median_flow(f, weight=cellw, cell_size=(16, 48)), expc)
    assert np.array_equal(outlier_mask(f, weight=cellw.astype(np.int64), cell_size=(16, 48)), keepc)
    # a FlowGrid stands for its flow and gives the kind of array its nodes are
    clean, _ = make_flow(H, W, noise=0.0)
    nodes = np.ascontiguousarray(clean[::8, ::8])
    grid = FlowGrid(nodes, 8, (H, W))
    expg, keepg, _ = R.median_flow_ref(grid.expand(), 2, None, None, "all", 1.0)
    out = median_flow(grid)
    assert isinstance(out, np.ndarray) and same_bits(out, expg)
    dgrid = FlowGrid(ctx.asdevice(nodes), 8, (H, W))
    out = median_flow(dgrid)
    assert isinstance(out, DeviceArray) and same_bits(out.numpy(), expg)
    assert np.array_equal(outlier_mask(grid), keepg) and isinstance(outlier_mask(dgrid), DeviceArray)


def test_out_and_keep_arrays_of_the_caller(ctx):
    f, rng = make_flow(50, 77)
    exp, exp_keep, counts = R.median_flow_ref(f, 2, None, None, "outliers", 0.3)
    d = ctx.asdevice(f)
    out, keep = ctx.empty(f.shape, F32), ctx.empty(f.shape[:2], np.uint8)
    got = ctx.median_flow(d, 2, where="outliers", thresh=0.3, out=out, keep=keep)
    assert got[0] is out and got[1] is keep and same_bits(out.numpy(), exp) and np.array_equal(keep.numpy(), exp_keep)
    assert ctx.median_flow(d, 2, where="outliers", thresh=0.3, out=out) is out
    # keep alone: no flow is written (out is NULL at the C level), through the context and through the C entry
    only = ctx.median_flow(d, 2, where="outliers", thresh=0.3, out=False, keep=True)
    assert isinstance(only, DeviceArray) and np.array_equal(only.numpy(), exp_keep)
    only, info = ctx.median_flow(d, 2, where="outliers", thresh=0.3, out=False, keep=True, return_info=True)
    assert np.array_equal(only.numpy(), exp_keep) and tuple(info) == counts
    keep2 = ctx.empty(f.shape[:2], np.uint8)
    ctx._run(ctx.lib.ma_median_flow, d.ptr, 50, 77, 2, None, 0, 1, 1, 1, 0.3, 0, None, keep2.ptr, None)
    assert np.array_equal(keep2.numpy(), exp_keep)
    with pytest.raises(ValueError):
        ctx.median_flow(d, 2, out=d)
    assert same_bits(d.numpy(), f)


# ---- refused arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_c_entry(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    f, rng = make_flow(H, W)
    d, out, keep = ctx.asdevice(f), ctx.empty(f.shape, F32), ctx.empty((H, W), np.uint8)
    w32, w8 = ctx.asdevice(np.ones((H, W), F32)), ctx.asdevice(np.ones((H, W), np.uint8))
    ok = dict(flow=d.ptr, H=H, W=W, r=2, weight=None, kind=0, ch=1, cw=1, mode=0, thresh=1.0, flags=0, out=out.ptr,
              keep=keep.ptr, counts=None)
    mf = lambda **kw: ctx._run(ctx.lib.ma_median_flow, *dict(ok, **kw).values())     # noqa: E731
    mf()
    mf(weight=w32.ptr, kind=1, mode=1, flags=1)
    mf(weight=w8.ptr, kind=2, ch=0, cw=-5)            # the cell size is read for the cell kind only
    mf(weight=w32.ptr, kind=3, ch=1000, cw=1000)
    mf(out=None)
    mf(keep=None, thresh=float("inf"), r=7)
    for kw in (dict(flow=None), dict(out=None, keep=None), dict(out=d.ptr), dict(H=0), dict(W=0), dict(H=-1), dict(H=big),
               dict(W=big), dict(H=1 << 24, W=1 << 24), dict(r=0), dict(r=-1), dict(r=8), dict(kind=-1), dict(kind=4), dict(kind=1), dict(kind=2),
               dict(kind=3), dict(mode=-1), dict(mode=2), dict(weight=w32.ptr, kind=3, ch=0, cw=4),
               dict(weight=w32.ptr, kind=3, ch=4, cw=0), dict(weight=w32.ptr, kind=3, ch=-1, cw=4), dict(thresh=-1.0),
               dict(thresh=float("nan")), dict(thresh=-float("inf")), dict(flags=2), dict(flags=3), dict(flags=-1),
               dict(weight=out.ptr, kind=1), dict(weight=keep.ptr, kind=2)):
        with pytest.raises(ValueError):
            mf(**kw)
    assert ctx.lib.ma_median_flow(None, *ok.values()) == _lib.MA_EINVAL
    assert ctx.lib.ma_median_flow(ctx.handle, *dict(ok, r=200).values()) == _lib.MA_EINVAL
    assert same_bits(d.numpy(), f)                                    # a refused call wrote nothing


def test_the_context_refuses_before_any_device_call(ctx, monkeypatch):
    f, _ = make_flow(20, 30)
    d = ctx.asdevice(f)
    w, w31, k8 = ctx.asdevice(np.ones((20, 30), F32)), ctx.asdevice(np.ones((20, 31), F32)), ctx.asdevice(np.ones((20, 31), np.uint8))
    calls = []
    monkeypatch.setattr(type(ctx), "_run", lambda self, fn, *a: calls.append(fn))
    monkeypatch.setattr(type(ctx), "empty", lambda self, *a: calls.append("empty"))
    for kw in (dict(radius=0), dict(radius=8), dict(radius=1.0), dict(where="blend"), dict(where="outliers"),
               dict(thresh=-1.0), dict(thresh=float("nan")), dict(weight=w31), dict(cell_size=5), dict(weight=w, cell_size=5),
               dict(flow=w), dict(out=w), dict(out=d), dict(keep=k8), dict(keep=w), dict(out=False), dict(generic=1)):
        with pytest.raises(ValueError):
            ctx.median_flow(**dict(dict(flow=d), **kw))
    assert calls == []


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    import microaligner_amd
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_median_flow"] == sorted(_lib.FLOWMEDIAN_SIGNATURES)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_flowmedian.h but not exported"
        proto = re.search(r"\b" + n + r"\s*\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.FLOWMEDIAN_SIGNATURES[n][1]) == 15, n
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES") and t != "FLOWMEDIAN_SIGNATURES"]
    assert len(others) >= 17 and not any(set(_lib.FLOWMEDIAN_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_flowsmooth.h"' in open(HEADER).read()            # the weight kinds are the smoothing's
    found = re.findall(r"\b(MA_[A-Z0-9_]+)\s*=?\s+(\d+)\b", text)
    assert sorted(n for n, _ in found) == ["MA_MEDIAN_ALL", "MA_MEDIAN_GENERIC", "MA_MEDIAN_MAX_RADIUS", "MA_MEDIAN_OUTLIERS"]
    for name, value in found:
        assert getattr(_lib, name) == int(value), name
    assert {"median_flow", "outlier_mask", "MedianInfo"} <= set(microaligner_amd.__all__)


def test_the_source_hash_is_the_parents(tmp_path, monkeypatch):
    """build.source_hash() reads the files and flags it read before this source existed: the library's hash is the tree's,
    and the hash taken with the new source and its headers struck from the build's lists -- what the parent commit computes
    from the same files -- is the same, as it is after an edit of the new source."""
    from microaligner_amd import build
    before = build.source_hash()
    assert _lib.source_hash() == before
    assert "flow_median.hip" in build.SOURCES and "microaligner_flowmedian.h" not in " ".join(build.HEADERS)
    own = [os.path.basename(h) for h in build.SOURCE_HEADERS["flow_median.hip"]]
    assert own == ["microaligner_flowmedian.h", "microaligner_flowsmooth.h", "weight_map.h", "call_counts.h"]
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "flow_median.hip"])
    monkeypatch.setattr(build, "SOURCE_HEADERS", {k: v for k, v in build.SOURCE_HEADERS.items() if k != "flow_median.hip"})
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
    with open(csrc / "flow_median.hip", "a") as fh:
        fh.write("\n// edited\n")
    assert build.source_hash() == before
    with open(csrc / "remap.hip", "a") as fh:
        fh.write("\n// edited\n")
    assert build.source_hash() != before
