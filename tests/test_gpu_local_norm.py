"""-m gpu: the local contrast normalisation on the device.  ma_normalize_local against the numpy float32 statement of
include/microaligner_localnorm.h (tests/_local_norm_ref.py) bit for bit, its counts exactly; normalize_local() end to end;
refused arguments at the C entry.  The refusals below the alignment rule are in tests/test_gpu_unaligned.py, the registry
cases (stale scratch memory, shifted addresses) in tests/_gpu_cases/local_norm.py.

Observed on an MI355X: every case gives the statement's bits and counts; the file takes 1.8 s."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_smooth_ref as S  # noqa: E402
import _local_norm_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402
from microaligner_amd import LocalNormInfo, _lib, normalize_local  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402
from test_gpu_flow_smooth import taps_of  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [np.uint8, np.uint16, np.float32]
# images smaller than r, one past the 64-line edge of a tile and one past its 128 outputs, either way
SHAPES = [(1, 1), (1, 300), (200, 1), (65, 129), (67, 301), (130, 70)]
WANTS = [("u8", "f32"), ("u8",), ("f32",)]


def same_bits(got, exp):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, got.shape, exp.dtype, exp.shape)
    if got.dtype != F32:
        return np.array_equal(got, exp)
    return not np.isnan(got).any() and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def check(ctx, img, taps, floor, clip=4.0, weight=None, min_support=0.0, wants=WANTS):
    """every set of outputs in `wants`, with the counts and without; -> the statement"""
    exp = R.normalize_local_ref(img, taps, floor, clip, weight, min_support)
    d_img = ctx.asdevice(img)
    d_w = None if weight is None else ctx.asdevice(weight)
    for k, want in enumerate(wants):
        got = ctx.normalize_local(d_img, taps, floor, clip, d_w, min_support, want, return_info=k % 2 == 0)
        if k % 2 == 0:
            got, info = got
            assert isinstance(info, LocalNormInfo) and tuple(info) == exp["counts"], (want, tuple(info), exp["counts"])
        assert tuple(got) == tuple(want)
        for n in want:
            assert same_bits(got[n].numpy(), exp[n]), (n, want)
    return exp


def weights_of(shape):
    w, mask = R.make_weight(*shape)
    return [(None, 0.0), (w, 0.3), (mask, 0.05)]


@pytest.mark.parametrize("r", [1, 7, 49, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_numpy_statement_bit_for_bit(ctx, shape, r):
    """u8, u16 and f32; no weight, a float32 weight with NaN, 0, negative and > 1 entries, a uint8 mask; each output alone
    and both together; the counts with and without"""
    taps = taps_of(r)
    assert len(taps) == r + 1
    for dtype in DTYPES:
        img = R.make_image(*shape, dtype)
        for k, (weight, ms) in enumerate(weights_of(shape)):
            exp = check(ctx, img, taps, R.floor_of(dtype), 2.0 if k == 1 else 4.0, weight, ms)
            assert sum(exp["counts"][:2]) + (~np.isnan(exp["z"])).sum() == img.size


def test_a_large_image(ctx):
    """(2049, 1031) uint16 at r = 21: many blocks either way; every count occurs"""
    img = R.make_image(2049, 1031, np.uint16)
    mask = np.ones(img.shape, np.uint8)
    mask[900:1100, 100:300] = 0
    mask[1000, 150:250:10] = 1          # lone live pixels in the hole: their windows hold t[0]^2 = 0.003 of weight
    exp = check(ctx, img, taps_of(21), R.floor_of(np.uint16), 2.0, mask, 0.02, wants=[("u8", "f32")])
    assert all(c > 0 for c in exp["counts"]), exp["counts"]


@pytest.mark.parametrize("r", [2, 18])
def test_nan_inf_and_extreme_pixels(ctx, r):
    """a non-finite pixel is dropped like a masked one and leaves its window supported; finite extremes overflow d d (v is
    +Inf and z is 0 across their windows) and, under a weight above 1, w x as well (mu is infinite, z is NaN: unsupported,
    no contrast); what the statement makes of either the kernels make too"""
    img = R.make_image(67, 301, np.float32)
    floor = R.floor_of(np.float32)
    clean = R.normalize_local_ref(img, taps_of(r), floor)
    img = img.copy()
    img[20, 40], img[50, 200], img[66, 300], img[0, 0] = np.nan, np.inf, -np.inf, np.nan
    exp = check(ctx, img, taps_of(r), floor)
    assert exp["counts"][:2] == (4, 0) and not np.array_equal(exp["f32"], clean["f32"])
    assert exp["u8"][20, 40] == 128 and exp["f32"][50, 200] == 0
    fmax = np.finfo(F32).max
    img[5, 5], img[40, 150], img[60, 20], img[60, 21] = fmax, -fmax, 1e30, 1e-38
    exp = check(ctx, img, taps_of(r), floor)
    assert exp["counts"][:2] == (4, 0) and np.isinf(exp["v"][5, 5]) and np.isinf(exp["v"][60, 20 - r])
    assert exp["z"][5, 5] == 0 and exp["u8"][5, 5 + r] == 128 and exp["f32"][40 - r, 150] == 0
    w = R.make_weight(*img.shape)[0]
    w[5, 5], w[40, 150] = 2.0, 1.5
    exp = check(ctx, img, taps_of(r), floor, 4.0, w, 0.3)
    assert np.isnan(exp["z"][5, 5]) and np.isnan(exp["z"][40, 150]) and exp["u8"][5, 5] == 128 and exp["f32"][40, 150] == 0
    assert (r + 1) ** 2 <= exp["counts"][R.UNSUPPORTED] < img.size // 4        # the live pixels of the two windows
    assert not np.isnan(exp["f32"]).any()


def test_a_fully_masked_image_and_a_support_above_every_sum(ctx):
    img = R.make_image(65, 129, np.uint8)
    for kw in (dict(weight=np.zeros(img.shape, np.uint8)), dict(weight=np.full(img.shape, np.nan, F32)), dict(min_support=1.5)):
        exp = check(ctx, img, taps_of(7), R.floor_of(np.uint8), **kw)
        assert (exp["u8"] == 128).all() and not exp["f32"].any() and not np.signbit(exp["f32"]).any()
        assert sum(exp["counts"][:2]) == img.size and exp["counts"][2:] == (0, 0)
        assert exp["counts"][R.DROPPED] == (0 if "min_support" in kw else img.size)


@pytest.mark.parametrize("scale", [1e-20, 3e-10])
def test_small_values(ctx, scale):
    """1e-20: d d (about 1e-42), its sums and the floor are denormal; 3e-10: they are about 1e-21, small and normal.  The
    outputs are those of the unscaled image up to rounding: z does not depend on the scale."""
    base = R.make_image(65, 129, np.float32)
    img = (base * F32(scale)).astype(F32)
    floor = float(F32(R.floor_of(np.float32)) * F32(scale) * F32(scale))
    tiny = np.finfo(F32).tiny
    assert 0 < floor < tiny if scale == 1e-20 else floor > tiny
    exp = check(ctx, img, taps_of(7), floor)
    ref = R.normalize_local_ref(base, taps_of(7), R.floor_of(np.float32))
    assert np.ptp(exp["u8"]) > 150 and exp["counts"][R.FLAT] > 0
    if scale == 3e-10:          # nothing is denormal: a few roundings apart, and a level is 2^-5 of z
        assert np.abs(exp["u8"].astype(np.int16) - ref["u8"].astype(np.int16)).max() <= 1


def test_clip_extremes(ctx):
    """+Inf with the float32 output alone: z itself.  1e30: the uint8 output is 128 everywhere there is contrast to speak of.
    1e-40: scale = 127 / clip overflows to +Inf, and z = 0 against it is a NaN sum that max takes to level 0."""
    img = R.make_image(67, 301, np.uint16)
    img[30, 100] = 65535                # a hot pixel: z is about 1 / t[0] = 5.5
    taps, floor = taps_of(7), R.floor_of(np.uint16)
    exp = check(ctx, img, taps, floor, np.inf, wants=[("f32",)])
    assert exp["u8"] is None and same_bits(exp["f32"], np.nan_to_num(exp["z"], nan=0.0)) and exp["counts"][R.CLIPPED] == 0
    assert np.abs(exp["f32"]).max() > 4
    exp = check(ctx, img, taps, floor, 1e30)
    assert (exp["u8"] == 128).all() and np.array_equal(exp["f32"], np.nan_to_num(exp["z"], nan=0.0))
    exp = check(ctx, img, taps, floor, 1e-40)
    assert set(np.unique(exp["u8"])) == {0, 255} and (exp["z"] == 0).any() and (exp["u8"][exp["z"] == 0] == 0).all()
    assert np.abs(exp["f32"]).max() == F32(1e-40) and exp["counts"][R.CLIPPED] > 0.9 * img.size


def test_a_small_call_after_a_large_one_on_the_same_context(ctx):
    """the workspace of the large call is the small call's stale scratch memory"""
    for r in (3, 128):
        big = R.make_image(420, 404, np.uint16)
        w, mask = R.make_weight(*big.shape)
        ctx.normalize_local(ctx.asdevice(big), taps_of(r), R.floor_of(np.uint16), 4.0, ctx.asdevice(w), 0.3, ("u8", "f32"))
        small = R.make_image(131, 157, np.float32)
        w, mask = R.make_weight(*small.shape)
        check(ctx, small, taps_of(r), R.floor_of(np.float32), 4.0, mask, 0.05, wants=[("u8", "f32")])
        check(ctx, small, taps_of(r), R.floor_of(np.float32), 4.0, w, 0.3, wants=[("f32",), ("u8",)])


def test_a_power_of_two_gain_changes_no_bit_on_the_device(ctx):
    img = R.make_image(67, 301, np.float32)
    w, _ = R.make_weight(*img.shape)
    taps, floor = taps_of(3), R.floor_of(np.float32)
    d_w = ctx.asdevice(w)
    a, ia = ctx.normalize_local(ctx.asdevice(img), taps, floor, 4.0, d_w, 0.3, ("u8", "f32"), return_info=True)
    b, ib = ctx.normalize_local(ctx.asdevice(img * F32(4)), taps, floor * 16, 4.0, d_w, 0.3, ("u8", "f32"), return_info=True)
    assert ia == ib and ia.flat > 0 and ia.dropped > 0 and ia.unsupported > 0
    for n in ("u8", "f32"):
        assert same_bits(a[n].numpy(), b[n].numpy()), n
    assert np.ptp(a["u8"].numpy()) > 150


# ---- normalize_local() -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_normalize_local_end_to_end(ctx, dtype):
    img = R.make_image(96, 161, dtype)
    w, mask = R.make_weight(*img.shape)
    floor = R.floor_of(dtype)
    exp = R.normalize_local_ref(img, S.gaussian_taps(16.0), floor)
    got = normalize_local(img, floor=floor)
    assert isinstance(got, np.ndarray) and same_bits(got, exp["u8"])
    got, info = normalize_local(img, floor=floor, dtype="float32", return_info=True)
    assert isinstance(got, np.ndarray) and same_bits(got, exp["f32"])
    assert isinstance(info, LocalNormInfo) and tuple(info) == exp["counts"]
    # device arrays in, a device array out with on_device; a weight, another window, clip and support
    exp = R.normalize_local_ref(img, S.gaussian_taps(2.0, 2.5), floor, 2.0, w, 0.3)
    d, info = normalize_local(ctx.asdevice(img), 2.0, floor=floor, clip=2.0, weight=ctx.asdevice(w), truncate=2.5, min_support=0.3,
                              on_device=True, return_info=True)
    assert isinstance(d, DeviceArray) and d.dtype == np.uint8 and same_bits(d.numpy(), exp["u8"]) and tuple(info) == exp["counts"]
    assert info.dropped > 0 and info.unsupported > 0 and info.clipped > 0
    got = normalize_local(ctx.asdevice(img), 2.0, floor=floor, clip=2.0, weight=w, truncate=2.5, min_support=0.3, dtype=np.float32)
    assert isinstance(got, np.ndarray) and same_bits(got, exp["f32"])
    exp = R.normalize_local_ref(img, S.gaussian_taps(4.0), floor, np.inf, mask)
    got = normalize_local(img, 4.0, floor=floor, clip=np.inf, weight=mask, dtype="float32", on_device=True)
    assert isinstance(got, DeviceArray) and same_bits(got.numpy(), exp["f32"])
    with pytest.raises(ValueError):
        normalize_local(img, 4.0, floor=floor, clip=np.inf)


def test_a_gain_field_comes_out(ctx):
    """the pair of the usefulness table: the moving image under a +-40 % gain and a +-30 level offset field normalises to
    within a few levels of what it normalises to without them, where min/max scaling leaves tens of levels"""
    from microaligner_amd import synthetic
    from oracle import oracle as O
    _, mov = synthetic.make_pair(512, 512, seed=1)
    g, o = R.gain_field(512, 512)
    gained = (mov * g + o + 40).astype(F32)
    a, b = (normalize_local(x, 16.0, floor=1.0).astype(np.int16) for x in (mov, gained))
    plain = np.abs(O.normalize_minmax_u8(mov).astype(np.int16) - O.normalize_minmax_u8(gained).astype(np.int16))
    diff = np.abs(a - b)[64:-64, 64:-64]
    print(f"levels between the clean and the gained image: normalised median {np.median(diff):.1f}, p99 {np.percentile(diff, 99):.1f}; "
          f"min/max median {np.median(plain):.1f}, p99 {np.percentile(plain, 99):.1f}")
    assert np.percentile(diff, 99) < np.median(plain[64:-64, 64:-64])


# ---- refused arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_c_entry(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    img = R.make_image(H, W, np.uint8)
    floor = R.floor_of(np.uint8)
    d_img = ctx.asdevice(img)
    f32, u8 = ctx.asdevice(np.full((H, W), 7, F32)), ctx.asdevice(np.full((H, W), 7, np.uint8))
    d_w = ctx.asdevice(np.ones((H, W), F32))
    counts = (C.c_longlong * 4)(-1, -1, -1, -1)
    taps = (C.c_float * 4)(0.4, 0.2, 0.1, 0.0)
    nan, inf = float("nan"), float("inf")

    def bad_taps(*v):
        return (C.c_float * len(v))(*v)
    ok = dict(img=d_img.ptr, dtype=0, H=H, W=W, taps=taps, r=3, floor=floor, clip=4.0, weight=d_w.ptr, kind=1, ms=0.0,
              f32=f32.ptr, u8=u8.ptr, counts=counts)
    ln = lambda **kw: ctx._run(ctx.lib.ma_normalize_local, *dict(ok, **kw).values())     # noqa: E731
    ln()
    exp = R.normalize_local_ref(img, np.array(taps[:], F32), floor)
    assert tuple(counts) == exp["counts"]
    # the weight pointer is ignored without a weight; either output alone; an infinite clip with the float32 output alone
    ln(weight=None, kind=0, counts=None)
    ln(weight=12345, kind=0, u8=None)
    ln(f32=None)
    ln(u8=None, clip=inf)
    ln()
    for kw in (dict(img=None), dict(taps=None), dict(f32=None, u8=None), dict(f32=u8.ptr), dict(u8=f32.ptr), dict(f32=d_img.ptr),
               dict(u8=d_img.ptr), dict(f32=d_w.ptr), dict(u8=d_w.ptr),
               dict(H=0), dict(W=0), dict(H=-1), dict(H=big), dict(W=big), dict(r=0), dict(r=-1), dict(r=129), dict(dtype=3),
               dict(dtype=-1), dict(taps=bad_taps(0.0, 0.2, 0.1, 0.0)), dict(taps=bad_taps(0.4, -0.2, 0.1, 0.0)),
               dict(taps=bad_taps(0.4, 0.2, nan, 0.0)), dict(taps=bad_taps(0.4, 0.2, 0.1, inf)),
               dict(floor=0.0), dict(floor=-1.0), dict(floor=nan), dict(floor=inf),
               dict(clip=0.0), dict(clip=-4.0), dict(clip=nan), dict(clip=-inf), dict(clip=inf), dict(clip=inf, f32=None),
               dict(ms=-0.5), dict(ms=nan), dict(ms=inf),
               dict(kind=3), dict(kind=-1), dict(kind=4), dict(weight=None), dict(weight=None, kind=2)):
        with pytest.raises(ValueError):
            ln(**kw)
    assert ctx.lib.ma_normalize_local(None, *ok.values()) == _lib.MA_EINVAL
    assert ctx.lib.ma_normalize_local(ctx.handle, *dict(ok, r=200).values()) == _lib.MA_EINVAL
    ctx.sync()
    assert same_bits(f32.numpy(), exp["f32"]) and same_bits(u8.numpy(), exp["u8"])     # a refused call wrote nothing
    assert tuple(counts) == exp["counts"]


def test_the_library_exports_the_entry_and_carries_the_parents_hash():
    from microaligner_amd import build
    lib = _lib.load()
    assert hasattr(lib, "ma_normalize_local"), "ma_normalize_local declared in microaligner_localnorm.h but not exported"
    assert build.source_hash() == HASH == _lib.source_hash()
