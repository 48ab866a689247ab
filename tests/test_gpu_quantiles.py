"""-m gpu: the order statistics and the range normalisation on the device (csrc/quantile.hip, include/microaligner_quantile.h)
against the numpy statement (tests/_quantile_ref.py): every comparison is array_equal or ==.  Shapes from one pixel to a few
blocks, the three dtypes, rank sets in any order, keys on the digit boundaries, float32 keys that differ in the lowest digit
only, non-finite values, contended bins, zeros left out; then normalize_percentile and max_project_and_normalize on top."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _quantile_ref as R  # noqa: E402
from microaligner_amd import NormalizeInfo, max_project_and_normalize, normalize_percentile  # noqa: E402
from microaligner_amd.device import DeviceArray, QuantileCounts  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (7, 13), (64, 65), (301, 517)]
DTYPES = [np.uint8, np.uint16, np.float32]
QSETS = [[0.0], [1.0], [0.5, 0.5], [0.999, 0.75, 0.5, 0.001], [0.0, 0.001, 0.01, 0.25, 0.5, 0.75, 0.999, 1.0]]
Q8 = QSETS[-1]


def image(shape, dtype, seed=0):
    rng = np.random.default_rng(seed + 17 * shape[0] + shape[1])
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if dtype == np.uint16:
        # half full-range noise, half a narrow band: ranks that share their first digit and ranks that do not
        a = rng.integers(0, 65536, shape)
        b = 200 + rng.poisson(30, shape)
        return np.where(rng.random(shape) < 0.5, a, b).astype(np.uint16)
    return (rng.standard_normal(shape) * np.where(rng.random(shape) < 0.5, 1e3, 1e-3)).astype(np.float32)


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def check(ctx, img, q, ignore_zeros=False):
    vals, counts = ctx.image_quantiles(ctx.asdevice(np.ascontiguousarray(img)), q, ignore_zeros=ignore_zeros)
    want, wcounts = R.image_quantiles(img, q, ignore_zeros)
    assert isinstance(counts, QuantileCounts) and tuple(counts) == wcounts, (tuple(counts), wcounts)
    assert vals.dtype == np.float64 and same(vals, want), (vals, want)
    return vals, counts


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantiles_equal_the_statement(ctx, shape, dtype):
    img = image(shape, dtype)
    for q in QSETS:
        check(ctx, img, q)
    check(ctx, img, Q8, ignore_zeros=True)
    vals, counts = check(ctx, img, [0.0, 1.0])
    assert vals[0] == float(img.min()) and vals[1] == float(img.max()) and counts.pop == img.size
    # twice the same bits
    d = ctx.asdevice(img)
    a, b = ctx.image_quantiles(d, Q8), ctx.image_quantiles(d, Q8)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16", "f32"])
def test_constant_and_contended_images(ctx, dtype):
    """300 x 300 equal keys pass a 16-bit counter and all land in one bin; 5 % other values break the runs."""
    const = np.full((300, 300), 201, dtype)
    vals, counts = check(ctx, const, Q8)
    assert (vals == 201.0).all() and counts == (90000, 0, 0)
    rng = np.random.default_rng(3)
    other = image((300, 300), dtype, seed=5)
    mixed = np.where(rng.random((300, 300)) < 0.05, other, const).astype(dtype)
    check(ctx, mixed, Q8)
    check(ctx, mixed, [0.94, 0.96, 0.02, 0.98])
    # alternating neighbours: no run is longer than one pixel
    alt = np.where((np.arange(90000) & 1).reshape(300, 300) == 1, 7, 201).astype(dtype)
    check(ctx, alt, [0.0, 0.49999, 0.5, 1.0])


def test_u16_keys_on_the_digit_boundaries(ctx):
    rng = np.random.default_rng(4)
    img = rng.choice(np.array([0, 255, 256, 257, 65535], np.uint16), (97, 131))
    check(ctx, img, Q8)
    check(ctx, img, [0.2, 0.4, 0.6, 0.8])
    check(ctx, img, Q8, ignore_zeros=True)
    for v in (0, 255, 256, 257, 65535):
        assert check(ctx, np.full((3, 5), v, np.uint16), [0.0, 0.5, 1.0])[0].tolist() == [float(v)] * 3


def test_f32_negatives_zeros_denormals_and_neighbouring_floats(ctx):
    rng = np.random.default_rng(5)
    neg = -np.abs(rng.standard_normal((33, 47))).astype(np.float32) * 100
    check(ctx, neg, Q8)
    zeros = np.where(rng.random((40, 50)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros[3, 4], zeros[7, 8] = -1.0, 1.0
    vals, _ = check(ctx, zeros, [0.0, 0.25, 0.5, 0.75, 1.0])
    assert vals.tolist() == [-1.0, 0.0, 0.0, 0.0, 1.0] and not np.signbit(vals[1:4]).any()
    _, counts = check(ctx, zeros, [0.0, 1.0], ignore_zeros=True)
    assert counts == (2, 0, zeros.size - 2)
    tiny = np.float32(1e-45)
    den = (rng.integers(-2000, 2000, (29, 31)).astype(np.float32) * tiny).astype(np.float32)
    assert np.abs(den[den != 0]).max() < np.finfo(np.float32).tiny
    check(ctx, den, Q8)
    check(ctx, den, Q8, ignore_zeros=True)
    chain = np.empty(3000, np.float32)
    chain[0] = np.float32(1234.5)
    for i in range(1, 3000):
        chain[i] = np.nextafter(chain[i - 1], np.float32(np.inf))
    chain = rng.permutation(chain).reshape(50, 60)
    vals, _ = check(ctx, chain, Q8)
    assert len(set(vals.tolist())) == 8
    check(ctx, -chain, [0.3333, 0.3334, 0.6666, 0.6667])
    both = np.concatenate([chain.ravel(), -chain.ravel(), den.ravel()]).astype(np.float32)
    check(ctx, both, Q8)


def test_f32_non_finite_values_are_left_out_and_counted(ctx):
    rng = np.random.default_rng(6)
    img = (rng.standard_normal((101, 103)) * 50).astype(np.float32)
    r = rng.random(img.shape)
    img[r < 0.03] = np.nan
    img[(r >= 0.03) & (r < 0.05)] = np.inf
    img[(r >= 0.05) & (r < 0.06)] = -np.inf
    vals, counts = check(ctx, img, Q8)
    assert counts.nonfinite == int((~np.isfinite(img)).sum()) > 0 and counts.pop + counts.nonfinite == img.size
    assert np.isfinite(vals).all()
    for fill in (np.nan, np.inf, -np.inf):
        vals, counts = check(ctx, np.full((9, 11), fill, np.float32), [0.0, 0.5, 1.0])
        assert np.isnan(vals).all() and counts == (0, 99, 0)
    one = np.full((9, 11), np.nan, np.float32)
    one[4, 5] = -3.5
    assert check(ctx, one, [0.0, 0.5, 1.0])[0].tolist() == [-3.5] * 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16", "f32"])
def test_ignore_zeros(ctx, dtype):
    rng = np.random.default_rng(7)
    img = np.zeros((200, 200), dtype)
    idx = rng.choice(img.size, 20, replace=False)                      # 99.95 % zeros
    img.flat[idx] = image((4, 5), dtype, seed=9).ravel()
    img.flat[idx[0]] = 9
    vals, counts = check(ctx, img, Q8, ignore_zeros=True)
    assert counts.zeros >= img.size - 20 and counts.pop == img.size - counts.zeros and counts.pop >= 1
    vals, _ = check(ctx, img, [0.0, 0.5, 0.999])
    assert (vals[1:] == 0.0).all() if dtype != np.float32 else vals[1] == 0.0
    vals, counts = check(ctx, np.zeros((31, 33), dtype), [0.0, 1.0], ignore_zeros=True)
    assert np.isnan(vals).all() and counts == (0, 0, 31 * 33)
    assert check(ctx, np.zeros((31, 33), dtype), [0.0, 1.0])[0].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16", "f32"])
def test_a_view_that_is_not_16_byte_aligned_takes_the_scalar_path(ctx, dtype):
    img = image((64, 65), dtype, seed=2)
    d = ctx.asdevice(img)
    item = np.dtype(dtype).itemsize
    for off in (1, 3):
        view = DeviceArray(ctx, (img.size - off,), dtype, d.ptr + off * item, 0, owner=False)
        vals, counts = ctx.image_quantiles(view, Q8)
        want, wcounts = R.image_quantiles(img.ravel()[off:], Q8)
        assert same(vals, want) and tuple(counts) == wcounts
        lo, hi = float(want[1]), float(want[-2])
        assert np.array_equal(ctx.normalize_range_u8(view, lo, hi).numpy(), R.normalize_range_u8(img.ravel()[off:], lo, hi))


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16", "f32"])
def test_range_normalisation(ctx, dtype):
    for shape in SHAPES + [(1, 2), (3, 3), (5, 9), (5, 407)]:           # n % 4 in {0, 1, 2, 3}
        img = image(shape, dtype, seed=1)
        d = ctx.asdevice(img)
        mn, mx = ctx.minmax(d)
        assert (mn, mx) == (float(img.min()), float(img.max()))
        got = ctx.normalize_range_u8(d, mn, mx)
        assert got.dtype == np.uint8 and got.shape == img.shape
        assert np.array_equal(got.numpy(), ctx.normalize_minmax_u8(d).numpy()), shape
        assert np.array_equal(got.numpy(), R.normalize_range_u8(img, mn, mx)), shape
        assert not ctx.normalize_range_u8(d, mx, mx).numpy().any() and not ctx.normalize_range_u8(d, mx, mn).numpy().any()
        # values outside [lo, hi] saturate
        (lo, hi), _ = R.image_quantiles(img, [0.25, 0.75])
        out = ctx.normalize_range_u8(d, lo, hi).numpy()
        assert np.array_equal(out, R.normalize_range_u8(img, lo, hi)), shape
        if hi > lo:
            assert (out[img <= lo] == 0).all() and (out[img >= hi] == 255).all()
    assert {s[0] * s[1] % 4 for s in SHAPES + [(1, 2), (3, 3), (5, 9), (5, 407)]} == {0, 1, 2, 3}


def test_range_normalisation_of_non_finite_and_huge_values(ctx):
    special = np.array([np.nan, np.inf, -np.inf, 1e38, -1e38, 0.0, 10.0, 5.0, 4.999, 10.0001, 2.5], np.float32)
    out = ctx.normalize_range_u8(ctx.asdevice(special), 0.0, 10.0).numpy()
    assert out[:4].tolist() == [0, 255, 0, 255]
    assert out.tolist() == [0, 255, 0, 255, 0, 0, 255, 128, 127, 255, 64] == R.normalize_range_u8(special, 0.0, 10.0).tolist()
    assert not ctx.normalize_range_u8(ctx.asdevice(special), 3.0, 3.0).numpy().any()
    big = np.tile(special, 37).reshape(37, 11)
    assert np.array_equal(ctx.normalize_range_u8(ctx.asdevice(big), -1e30, 1e30).numpy(), R.normalize_range_u8(big, -1e30, 1e30))
    with pytest.raises(ValueError):
        ctx.normalize_range_u8(ctx.asdevice(special), float("nan"), 1.0)
    with pytest.raises(ValueError):
        ctx.image_quantiles(ctx.asdevice(special), [1.5])


def test_normalize_percentile_and_the_projection(ctx):
    hot = R.hot_pixel_image()
    out, info = normalize_percentile(hot, return_info=True)
    want, winfo = R.normalize_percentile(hot, 0.0, 99.9)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, want)
    assert isinstance(info, NormalizeInfo)
    for field in ("lo", "hi", "pop", "nonfinite", "zeros", "degenerate"):
        assert getattr(info, field) == winfo[field], field
    assert len(np.unique(out)) > 128 and len(np.unique(ctx.normalize_minmax_u8(ctx.asdevice(hot)).numpy())) < 16
    dev = normalize_percentile(ctx.asdevice(hot), 1.0, 99.0, on_device=True)
    assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), R.normalize_percentile(hot, 1.0, 99.0)[0])
    assert np.array_equal(normalize_percentile(hot, 0, 100), ctx.normalize_minmax_u8(ctx.asdevice(hot)).numpy())
    # data never raises: a constant image, an image that is all background below `high`, an empty population
    for img, kw in ((np.full((20, 30), 5, np.uint16), {}), (np.zeros((20, 30), np.float32), dict(ignore_zeros=True)),
                    (np.full((20, 30), np.nan, np.float32), {})):
        out, info = normalize_percentile(img, return_info=True, **kw)
        want, winfo = R.normalize_percentile(img, 0.0, 99.9, **kw)
        assert info.degenerate and not out.any() and np.array_equal(out, want)
        assert (info.pop, info.nonfinite, info.zeros) == (winfo["pop"], winfo["nonfinite"], winfo["zeros"])
        assert same([info.lo, info.hi], [winfo["lo"], winfo["hi"]])
    sparse = np.zeros((100, 100), np.uint16)
    sparse[10:12, 10:15] = np.arange(10, dtype=np.uint16).reshape(2, 5) * 100 + 50
    out, info = normalize_percentile(sparse, 0, 99.9, return_info=True)          # > 99.9 % background: black, and flagged
    assert info.degenerate and not out.any()
    out, info = normalize_percentile(sparse, 0, 99.9, ignore_zeros=True, return_info=True)
    assert not info.degenerate and (info.lo, info.hi, info.pop, info.zeros) == (50.0, 850.0, 10, 9990)
    assert np.array_equal(out, R.normalize_percentile(sparse, 0, 99.9, ignore_zeros=True)[0])
    # three pages: the projection, then the statement
    rng = np.random.default_rng(8)
    pages = np.stack([hot, rng.permutation(hot.ravel()).reshape(hot.shape), (hot // 2).astype(np.uint16)])
    proj = np.maximum.reduce(list(pages))
    got, info = max_project_and_normalize(pages, percentiles=(0, 99.9), return_info=True)
    want, winfo = R.normalize_percentile(proj, 0.0, 99.9)
    assert np.array_equal(got, want) and (info.lo, info.hi, info.pop) == (winfo["lo"], winfo["hi"], winfo["pop"])
    dev = max_project_and_normalize(pages, on_device=True, percentiles=(2, 98), ignore_zeros=True)
    assert isinstance(dev, DeviceArray) and np.array_equal(dev.numpy(), R.normalize_percentile(proj, 2, 98, ignore_zeros=True)[0])
    # percentiles=None is today's output
    today = ctx.normalize_minmax_u8(ctx.max_project(ctx.asdevice(pages))).numpy()
    assert np.array_equal(max_project_and_normalize(pages), today)
    assert np.array_equal(max_project_and_normalize(pages, percentiles=None), today)
    assert np.array_equal(today, R.normalize_range_u8(proj, float(proj.min()), float(proj.max())))
