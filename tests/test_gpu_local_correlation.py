"""-m gpu: the local correlation maps on the device.  ma_local_correlation against the numpy float32 statement of
include/microaligner_localcorr.h (tests/_local_correlation_ref.py) bit for bit, its counts exactly; local_correlation() end
to end; the weight in its consumers; refused arguments at the C entry."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_smooth_ref as S  # noqa: E402
import _local_correlation_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402
from microaligner_amd import CorrelationMaps, FlowGrid, _lib, fit_flow_affine, local_correlation, smooth_flow  # noqa: E402
from microaligner_amd.device import DeviceArray, grid_nodes  # noqa: E402
from test_gpu_flow_invert import same_bits  # noqa: E402
from test_gpu_flow_smooth import SHAPES, taps_of  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [np.uint8, np.uint16, np.float32]
CELLS = (16, 48)
SMALL = [(1, 1), (1, 300), (300, 1), (7, 5)]
PLANES = ("score", "weight")


def make_pair(H, W, dtype, seed=0):
    """(ref of dtype, the other image float32 in ref's grey levels, floor): noise and a cosine under a smooth envelope that
    is exactly 0 in the lower right part (flat); the other image is 0.8 ref + 0.05 with a little noise of its own (agree),
    but in the upper right quarter it has noise of its own under the envelope (disagree)"""
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    env = np.clip(1.2 - (x / max(W - 1, 1)) ** 2 - (y / max(H - 1, 1)) ** 2, 0, 1)
    v = 0.5 + 0.5 * env * (0.6 * rng.random((H, W)) + 0.4 * np.cos(x / 3.0) - 0.5)
    o = 0.8 * v + 0.05 + 0.01 * env * rng.normal(0, 1, (H, W))
    other = 0.45 + 0.4 * env * (rng.random((H, W)) - 0.5)
    o[:H // 2, W // 2:] = other[:H // 2, W // 2:]
    full = R.full_scale(dtype)
    return R.quantise(v, dtype), (o * full).astype(F32), (0.02 * full) ** 2


def make_weight(H, W, seed=0):
    """a float32 weight with NaN, 0, negative and > 1 entries, and a uint8 mask with a hole"""
    rng = np.random.default_rng(77 * H + W + seed)
    w = rng.uniform(0.1, 2.5, (H, W)).astype(F32)
    pick = rng.random((H, W))
    w[pick < 0.04], w[(pick >= 0.04) & (pick < 0.08)], w[(pick >= 0.08) & (pick < 0.12)] = np.nan, 0.0, -1.0
    w[:, W // 3:W // 3 + max(1, W // 5)] = 0.0
    mask = (rng.random((H, W)) < 0.9).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
    mask[H // 4:H // 4 + max(1, H // 3)] = 0
    return w, mask


def centres(ref, img):
    fin = img[np.isfinite(img)]
    r = np.asarray(ref, F32)
    r = r[np.isfinite(r)]
    return (float(F32(np.median(r))) if r.size else 0.0, float(F32(np.median(fin))) if fin.size else 0.0)


def check(ctx, ref, img, taps, floor, cells_list, center=(0.0, 0.0), weight=None, alone=True, **kw):
    """all outputs together per cell size, and with `alone` each output alone; -> the statement"""
    exp = R.local_correlation_ref(ref, img, taps, floor, center, weight, cell_size=cells_list[0], **kw)
    d_ref, d_img = ctx.asdevice(ref), ctx.asdevice(img)
    d_w = None if weight is None else ctx.asdevice(weight)
    run = lambda cells, want: ctx.local_correlation(d_ref, d_img, taps, floor, center, d_w, cell_size=cells, want=want, **kw)  # noqa: E731
    for cells in cells_list:
        got = run(cells, PLANES)
        for n in PLANES:
            assert same_bits(got[n].numpy(), exp[n]), n
        assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], R.cell_counts(exp["classes"], cells))
    if alone:
        for n in PLANES:
            got = run(None, (n,))
            assert list(got) == [n] and same_bits(got[n].numpy(), exp[n]), n
        got = run(cells_list[0], ())
        assert list(got) == ["counts"] and np.array_equal(got["counts"], exp["counts"])
    return exp


@pytest.mark.parametrize("r", [1, 7, 49, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_numpy_statement_bit_for_bit(ctx, shape, r):
    """u8, u16 and f32; no weight, a float32 weight with NaN, 0, negative and > 1 entries, a uint8 mask; centred and
    uncentred; every output alone and all together; cells (16, 48), one cell, and (1, 1) on the small shapes; images smaller
    than r are among the shapes"""
    taps = taps_of(r)
    assert len(taps) == r + 1
    cells_list = [CELLS, (1000, 1000)] + ([(1, 1)] if shape in SMALL else [])
    w, mask = make_weight(*shape)
    for k, dtype in enumerate(DTYPES):
        ref, img, floor = make_pair(*shape, dtype)
        c = centres(ref, img)
        check(ctx, ref, img, taps, floor, cells_list, c)
        check(ctx, ref, img, taps, floor, [CELLS], (0.0, 0.0), alone=False)
        check(ctx, ref, img, taps, floor, [CELLS], c if k == 1 else (0.0, 0.0), w, alone=k == 0, min_support=0.3, lo=-0.5, hi=0.9)
        check(ctx, ref, img, taps, floor, [CELLS], (0.0, 0.0) if k == 1 else c, mask, alone=k == 2, min_support=0.05)


def test_a_large_image(ctx):
    """(2049, 1031) uint16 at r = 21: many blocks either way; all four classes occur"""
    ref, img, floor = make_pair(2049, 1031, np.uint16)
    mask = np.ones(ref.shape, np.uint8)
    mask[900:1100, 100:300] = 0
    exp = check(ctx, ref, img, taps_of(21), floor, [(100, 100)], centres(ref, img), mask, alone=False)
    assert (exp["counts"].sum((0, 1)) > 0).all()


@pytest.mark.parametrize("r", [2, 18])
def test_nan_inf_and_extreme_pixels_in_either_image(ctx, r):
    """a non-finite pixel is dropped like a masked one; finite extremes overflow the products, and what the statement
    makes of that (NaN scores: unsupported) the kernels make too"""
    ref, img, floor = make_pair(67, 301, np.float32)
    clean = R.local_correlation_ref(ref, img, taps_of(r), floor)
    ref, img = ref.copy(), img.copy()
    ref[20, 40], ref[50, 200], ref[66, 300] = np.nan, np.inf, -np.inf
    img[10, 100], img[30, 250], img[0, 0] = np.nan, -np.inf, np.inf
    exp = check(ctx, ref, img, taps_of(r), floor, [CELLS], (0.25, 0.5))
    assert not np.isnan(exp["score"]).any()                       # dropped pixels leave their windows supported
    assert np.isfinite(clean["score"]).all() and not np.array_equal(exp["score"], clean["score"])
    ref[5, 5], img[40, 150], ref[60, 20], img[60, 21] = 3e38, -3e38, 1e30, 1e-38
    exp = check(ctx, ref, img, taps_of(r), floor, [CELLS], (0.25, 0.5))
    bad = np.isnan(exp["score"])
    assert bad[5, 5] and bad[40, 150] and 0 < bad.sum() < bad.size
    assert (exp["classes"][bad] == R.UNSUPPORTED).all() and not exp["weight"][bad].any()
    assert (exp["classes"][~bad] != R.UNSUPPORTED).all() and (exp["classes"] == R.FLAT).any()


def test_a_fully_masked_image_and_a_support_above_every_sum(ctx):
    ref, img, floor = make_pair(65, 129, np.uint8)
    for kw in (dict(weight=np.zeros(ref.shape, np.uint8)), dict(weight=np.full(ref.shape, np.nan, F32)), dict(min_support=1.5)):
        exp = check(ctx, ref, img, taps_of(7), floor, [CELLS], **kw)
        assert np.isnan(exp["score"]).all() and not exp["weight"].any()
        assert exp["counts"][..., R.UNSUPPORTED].sum() == ref.size == exp["counts"].sum()


@pytest.mark.parametrize("scale", [1e-20, 3e-10])
def test_denormal_scale_images(ctx, scale):
    """1e-20: the second-order products (about 1e-40), their sums and the floor are denormal; 3e-10: they are about 1e-20,
    small and normal"""
    ref, img, _ = make_pair(65, 129, np.float32)
    ref, img = (ref * F32(scale)).astype(F32), (img * F32(scale)).astype(F32)
    floor = float(F32(4e-4) * F32(scale) * F32(scale))
    exp = check(ctx, ref, img, taps_of(7), floor, [CELLS])
    S_ = R.sums(ref, img, taps_of(7))
    tiny = np.finfo(F32).tiny
    assert 0 < S_[3].max() < tiny if scale == 1e-20 else S_[3].max() > tiny
    assert np.isfinite(exp["score"]).all() and (exp["classes"] == R.AGREE).any() and (exp["classes"] == R.FLAT).any()


# ---- local_correlation() ---------------------------------------------------------------------------------------------------
H2, W2 = 96, 161


@functools.lru_cache(maxsize=None)
def e2e_pair(dtype):
    """the CPU test's pair displaced by a smooth 2 px flow: (ref, mov, flow, floor); mov warped by the flow is the other
    image of R.pair up to the interpolation"""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H2, 0:W2].astype(F64)
    u, v = 2.0 * np.cos(y / 40.0), 2.0 * np.sin(x / 50.0)
    full = R.full_scale(dtype)
    ref = R.quantise(R.values(H2, W2) + rng.normal(0, R.NOISE, (H2, W2)), dtype)
    o = R.values(H2, W2, u, v)
    o[R.BLOCK] = R.values(H2, W2, u + R.BLOCK_SHIFT, v)[R.BLOCK]
    mov = R.quantise(0.8 * o + 0.05 + rng.normal(0, R.NOISE, (H2, W2)), dtype)
    return ref, mov, np.stack([u, v], -1).astype(F32), 4 * (R.NOISE * full) ** 2


def statement_of(ctx, ref, warped, maps, floor, sigma=2.0, **kw):
    """the statement over the images the kernel saw, with the centres the call reports"""
    return R.local_correlation_ref(ref, warped, S.gaussian_taps(sigma), floor, maps.center, **kw)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_local_correlation_end_to_end(ctx, dtype):
    ref, mov, flow, floor = e2e_pair(dtype)
    maps = local_correlation(ref, mov, flow, floor=floor, sigma=2.0, cell_size=(32, 81))
    assert isinstance(maps, CorrelationMaps) and isinstance(maps.score, np.ndarray) and isinstance(maps.weight, np.ndarray)
    warped = ctx.warp_affine_flow(ctx.to_f32(ctx.asdevice(mov)), ctx.asdevice(flow), ((1, 0, 0), (0, 1, 0)), "linear").numpy()
    # the centres are the exact medians (numpy's method="lower") of what the kernel saw
    assert maps.center == (float(F32(np.quantile(ref, 0.5, method="lower"))), float(F32(np.quantile(warped, 0.5, method="lower"))))
    exp = statement_of(ctx, ref, warped, maps, floor, cell_size=(32, 81))
    assert same_bits(maps.score, exp["score"]) and same_bits(maps.weight, exp["weight"])
    for k, n in enumerate(("agree", "disagree", "flat", "unsupported")):
        assert getattr(maps, n).dtype == np.int64 and np.array_equal(getattr(maps, n), exp["counts"][..., k])
    assert maps.cell_bounds.shape == (3, 2, 4) and tuple(maps.cell_bounds[2, 1]) == (64, 96, 81, 161)
    s = maps.summary()
    assert s["pixels"] == H2 * W2 and s["cells"] == 6 and abs(s["agree"] + s["disagree"] + s["flat"] + s["unsupported"] - 1) < 1e-12
    assert s["worst_cell"] == (1, 0)                      # the block's: 0.34 of it against 0.27 where the warp's zero fill is
    # device arrays in, device arrays out, the same bits; without cell_size no counts
    d = local_correlation(ctx.asdevice(ref), ctx.asdevice(mov), ctx.asdevice(flow), floor=floor, sigma=2.0)
    assert isinstance(d.score, DeviceArray) and isinstance(d.weight, DeviceArray) and d.agree is None and d.cell_bounds is None
    assert same_bits(d.score.numpy(), maps.score) and same_bits(d.weight.numpy(), maps.weight)
    with pytest.raises(ValueError):
        d.summary()
    # the map before the registration: the images as they are
    before = local_correlation(ref, mov, floor=floor, sigma=2.0)
    mov32 = np.asarray(mov).astype(F32)
    exp0 = statement_of(ctx, ref, mov32, before, floor)
    assert same_bits(before.score, exp0["score"]) and same_bits(before.weight, exp0["weight"])
    tex, blk, _ = R.regions(H2, W2, 6)
    print(f"{np.dtype(dtype).name}: median score outside the block {np.median(maps.score[tex]):.3f} with the flow, "
          f"{np.median(before.score[tex]):.3f} without; inside {np.median(maps.score[blk]):.3f} / {np.median(before.score[blk]):.3f}")
    assert np.median(maps.score[tex]) > np.median(before.score[tex])
    assert np.median(maps.score[tex]) > 0.75
    assert (exp["classes"][blk] == R.DISAGREE).all() and (exp0["classes"][blk] == R.DISAGREE).all()
    # given centres, no centres, a weight, other thresholds
    mask = np.ones((H2, W2), np.uint8)
    mask[:, :30] = 0
    got = local_correlation(ref, mov, flow, floor=floor, sigma=2.0, center=None, weight=mask, lo=0.0, hi=0.5, min_support=0.1)
    exp = R.local_correlation_ref(ref, warped, S.gaussian_taps(2.0), floor, (0.0, 0.0), mask, 0.0, 0.5, 0.1)
    assert got.center == (0.0, 0.0) and same_bits(got.score, exp["score"]) and same_bits(got.weight, exp["weight"])
    got = local_correlation(ref, mov, flow, floor=floor, sigma=2.0, center=(3.5, -2.0))
    exp = R.local_correlation_ref(ref, warped, S.gaussian_taps(2.0), floor, (3.5, -2.0))
    assert got.center == (3.5, -2.0) and same_bits(got.score, exp["score"])


def test_dog_labels_a_flow_grid_and_a_matrix(ctx):
    ref, mov, flow, floor = e2e_pair(np.uint16)
    l_ref, l_mov = (ctx.dog_u8(ctx.asdevice(a), 5, 9) for a in (ref, mov))
    assert l_ref.dtype == np.uint8
    tmat = np.array([[1.0, 0.0, 0.75], [0.0, 1.0, -0.5]])
    warped = ctx.warp_affine_flow(ctx.to_f32(l_mov), ctx.asdevice(flow), tmat, "linear").numpy()
    got = local_correlation(ref, mov, flow, floor=4.0, tmat=tmat, sigma=2.0, labels="dog", cell_size=40)
    exp = statement_of(ctx, l_ref.numpy(), warped, got, 4.0, cell_size=(40, 40))
    assert same_bits(got.score, exp["score"]) and same_bits(got.weight, exp["weight"]) and np.array_equal(got.flat, exp["counts"][..., 2])
    same = local_correlation(l_ref.numpy(), l_mov.numpy(), flow, floor=4.0, tmat=tmat, sigma=2.0)
    assert same_bits(same.score, got.score)
    # a FlowGrid is its expansion; a matrix alone is a zero flow
    nodes = np.random.default_rng(3).normal(0, 0.4, (grid_nodes(H2, 16), grid_nodes(W2, 16), 2)).astype(F32)
    grid = FlowGrid(nodes, 16, ref.shape)
    a = local_correlation(ref, mov, grid, floor=floor, sigma=2.0)
    b = local_correlation(ref, mov, grid.expand(), floor=floor, sigma=2.0)
    assert isinstance(a.score, np.ndarray) and same_bits(a.score, b.score) and same_bits(a.weight, b.weight)
    warped = ctx.warp_affine_flow(ctx.to_f32(ctx.asdevice(mov)), ctx.asdevice(grid.expand()), ((1, 0, 0), (0, 1, 0)), "linear").numpy()
    assert same_bits(a.score, statement_of(ctx, ref, warped, a, floor)["score"])
    a = local_correlation(ref, mov, floor=floor, tmat=tmat, sigma=2.0)
    b = local_correlation(ref, mov, np.zeros((H2, W2, 2), F32), floor=floor, tmat=tmat, sigma=2.0)
    assert same_bits(a.score, b.score) and not same_bits(a.score, local_correlation(ref, mov, floor=floor, sigma=2.0).score)


def test_the_weight_feeds_the_consumers_as_it_is(ctx):
    ref, mov, flow, floor = e2e_pair(np.uint16)
    blk = R.regions(H2, W2, 6)[1]
    for kind in (np.asarray, ctx.asdevice):
        maps = local_correlation(kind(ref), kind(mov), kind(flow), floor=floor, sigma=2.0)
        w = maps.weight
        assert w.dtype == np.float32 and tuple(w.shape) == (H2, W2)
        host = w if isinstance(w, np.ndarray) else w.numpy()
        assert host.min() == 0 and host.max() == 1 and 0 < host.mean() < 1
        tmat = fit_flow_affine(kind(flow), weight=w)
        assert tmat.shape == (2, 3) and np.isfinite(tmat).all()
        out = smooth_flow(kind(flow), 2.0, weight=w, where="blend")
        out = out if isinstance(out, np.ndarray) else out.numpy()
        assert out.shape == (H2, W2, 2) and np.isfinite(out[host > 0]).all()      # NaN only deep in the constant part
        deep = R.regions(H2, W2, 16)[0]            # every weight within the smoothing's window is 1: blend keeps the flow
        assert deep.sum() > 1000 and np.array_equal(out[deep], flow[deep]) and not np.array_equal(out[blk], flow[blk])


# ---- refused arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_c_entry(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    ref, img, floor = make_pair(H, W, np.uint8)
    d_ref, d_img = ctx.asdevice(ref), ctx.asdevice(img)
    sc, wt = (ctx.asdevice(np.full((H, W), 7, F32)) for _ in range(2))
    d_w = ctx.asdevice(np.ones((H, W), F32))
    counts = (C.c_longlong * (4 * 2 * 4))()
    taps = (C.c_float * 4)(0.4, 0.2, 0.1, 0.0)
    nan, inf = float("nan"), float("inf")

    def bad_taps(*v):
        return (C.c_float * len(v))(*v)
    ok = dict(ref=d_ref.ptr, dtype=0, img=d_img.ptr, H=H, W=W, taps=taps, r=3, ca=100.0, cb=90.0, floor=floor, weight=d_w.ptr,
              kind=1, ms=0.0, lo=0.25, hi=0.75, score=sc.ptr, wt=wt.ptr, ch=16, cw=48, counts=counts)
    lc = lambda **kw: ctx._run(ctx.lib.ma_local_correlation, *dict(ok, **kw).values())     # noqa: E731
    lc()
    assert sum(counts) == H * W
    # the weight pointer is ignored without a weight, the cell size is read only with the counts
    lc(weight=None, kind=0, counts=None, ch=0, cw=-3)
    lc(score=None, wt=None, ch=1000, cw=1000)
    lc(lo=-1.0, hi=1.0)
    for kw in (dict(ref=None), dict(img=None), dict(taps=None), dict(score=None, wt=None, counts=None), dict(wt=sc.ptr),
               dict(H=0), dict(W=0), dict(H=-1), dict(H=big), dict(W=big), dict(r=0), dict(r=-1), dict(r=129), dict(dtype=3),
               dict(dtype=-1), dict(taps=bad_taps(0.0, 0.2, 0.1, 0.0)), dict(taps=bad_taps(0.4, -0.2, 0.1, 0.0)),
               dict(taps=bad_taps(0.4, 0.2, nan, 0.0)), dict(taps=bad_taps(0.4, 0.2, 0.1, inf)),
               dict(ca=nan), dict(ca=inf), dict(cb=nan), dict(cb=-inf),
               dict(floor=0.0), dict(floor=-1.0), dict(floor=nan), dict(floor=inf),
               dict(ms=-0.5), dict(ms=nan), dict(ms=inf),
               dict(lo=0.75), dict(lo=0.8), dict(lo=-1.5), dict(hi=1.5), dict(lo=nan), dict(hi=nan),
               dict(kind=3), dict(kind=-1), dict(kind=4), dict(weight=None), dict(weight=None, kind=2),
               dict(ch=0), dict(cw=0), dict(ch=-1)):
        with pytest.raises(ValueError):
            lc(**kw)
    assert ctx.lib.ma_local_correlation(None, *ok.values()) == _lib.MA_EINVAL
    assert ctx.lib.ma_local_correlation(ctx.handle, *dict(ok, r=200).values()) == _lib.MA_EINVAL
    ctx.sync()
    exp = R.local_correlation_ref(ref, img, np.array(taps[:], F32), floor, (100.0, 90.0), lo=-1.0, hi=1.0)
    assert same_bits(sc.numpy(), exp["score"]) and same_bits(wt.numpy(), exp["weight"])     # a refused call wrote nothing


def test_the_library_exports_the_entry_and_carries_the_parents_hash():
    from microaligner_amd import build
    lib = _lib.load()
    assert hasattr(lib, "ma_local_correlation"), "ma_local_correlation declared in microaligner_localcorr.h but not exported"
    assert build.source_hash() == HASH == _lib.source_hash()
