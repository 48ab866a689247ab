"""-m gpu: Context.morphology against the numpy statement of tests/_morph_ref.py, bit for bit (float32 compared as uint32):
there is no tolerance anywhere, an order statistic has no rounding and a hat is one subtraction.

The radii are the issue's grid and every radius at which csrc/morphology.hip changes what it does, with its neighbours:
  7 | 8    an output reads its 2 r + 1 taps (r <= MO_DIRECT_MAX = 7) | suffix, middle and prefix (r >= 8);
  15 | 16  the middle is single keys (k = r / 16 = 0) | block minima appear (k >= 1), and the halo is one block up to r = 16;
  16 | 17, 32 | 33  the halo grows by a block;  r = 16 k exactly (16, 32, 240): no single keys beside the block minima;
  96 | 97  the dynamic LDS of a launch (mo_lds) reaches 64 KiB, what a kernel has without asking: from r = 97 (exactly
           65536 bytes for r = 97 .. 112) mo_launch raises the kernel's limit first;  112 | 113  the first size above 64 KiB;
  255      the largest radius: 102 KiB of LDS.
There is no packed / unpacked switch and no split of the radius: one kernel for all dtypes and radii.
The shapes stand one below, at and one above the edges of its tile of 32 lines x 256 outputs, in both passes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _morph_ref as R  # noqa: E402

# The registry cases of ma_morphology (tests/_gpu_cases/morphology.py) register when that module is imported.  The package's
# own list of area modules does not name it, so this module imports it: it is collected before tests/test_gpu_stale_memory.py
# and tests/test_gpu_unaligned.py, which parametrise over the registry as it stands when they are imported.
pytest.register_assert_rewrite("_gpu_cases")
import _gpu_cases.morphology  # noqa: E402,F401

pytestmark = pytest.mark.gpu
ids = lambda d: np.dtype(d).name  # noqa: E731

ISSUE_RADII = [(0, 0), (0, 3), (3, 0), (1, 1), (2, 5), (7, 7), (31, 32), (64, 1), (255, 255)]
PATH_RADII = [(6, 8), (8, 7), (9, 15), (15, 16), (16, 17), (17, 14), (32, 33), (33, 240), (240, 127), (128, 254),
              (96, 97), (97, 96), (112, 113), (113, 112)]


def same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    bad = R.bits(got) != R.bits(exp)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:5].tolist()}"


def check_all_ops(ctx, img, radius, ops=R.OPS):
    exp = R.all_ops_ref(img, radius)
    d = ctx.asdevice(img)
    for op in ops:
        same(ctx.morphology(d, op, radius).numpy(), exp[op], f"{op} r={radius} {img.dtype} {img.shape}")


@pytest.mark.parametrize("radius", ISSUE_RADII + PATH_RADII, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_every_op_at_the_radii(ctx, dtype, radius):
    check_all_ops(ctx, R.make_image(263, 301, dtype, 21), radius)      # two tiles along either pass, ragged in both


SHAPES = [(1, 1), (1, 300), (200, 1), (65, 129), (67, 301), (130, 70),
          (31, 255), (32, 256), (33, 257), (255, 31), (256, 32), (257, 33)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_shapes_around_the_tile_edges(ctx, dtype, shape):
    img = R.make_image(*shape, dtype, 22)
    check_all_ops(ctx, img, (2, 3))
    check_all_ops(ctx, img, (9, 20))


@pytest.mark.parametrize("shape", [(40, 600), (600, 40)], ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_images_smaller_than_the_radius(ctx, dtype, shape):
    check_all_ops(ctx, R.make_image(*shape, dtype, 23), 255)


@pytest.mark.parametrize("dtype, ops", [(np.uint8, ("open",)), (np.uint16, ("erode",)), (np.float32, ("tophat",))],
                         ids=["uint8-open", "uint16-erode", "float32-tophat"])
def test_a_larger_image(ctx, dtype, ops):
    check_all_ops(ctx, R.make_image(2049, 1031, dtype, 24), 21, ops)


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_in_place(ctx, dtype, op):
    img = R.make_image(140, 300, dtype, 25)
    for radius in ((3, 2), (20, 11)):
        work = ctx.asdevice(img).copy()
        out = ctx.morphology(work, op, radius, out=work)
        assert out is work
        same(out.numpy(), R.morphology_ref(img, op, radius), f"{op} in place r={radius}")
    with pytest.raises(ValueError):
        ctx.morphology(ctx.asdevice(img), op, 1, out=ctx.empty((140, 300), np.float64))
    with pytest.raises(ValueError):
        ctx.morphology(ctx.asdevice(img), op, 1, out=ctx.empty((140, 301), dtype))


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=ids)
def test_integer_extremes(ctx, dtype):
    top = np.iinfo(dtype).max
    rng = np.random.default_rng(26)
    img = rng.choice(np.array([0, 1, top - 1, top], dtype), (90, 280), p=[0.4, 0.1, 0.1, 0.4])
    img[30:60, 100:200] = top
    img[5:20, 10:90] = 0
    for radius in ((1, 1), (4, 9), (16, 3)):
        check_all_ops(ctx, img, radius)


def test_float_special_values(ctx):
    rng = np.random.default_rng(27)
    img = R.SPECIALS[rng.integers(0, R.SPECIALS.size, (70, 290))]          # nothing but NaNs, +-Inf, +-0, denormals, +-FLT_MAX
    img[20:50, 40:120] = R.SPECIALS[rng.integers(0, 7, (30, 80))]          # windows of nothing but NaNs, both signs, payloads
    img[55:65, 200:260] = np.inf                                           # Inf - Inf in the hats
    img[0:8, 270:290] = -np.inf
    for radius in ((0, 0), (1, 1), (3, 8), (9, 17)):
        check_all_ops(ctx, img, radius)
    exp = R.all_ops_ref(img, (3, 8))
    assert (R.bits(exp["erode"])[25:45, 50:110] == 0x7fc00000).all()       # the cases are there
    assert (R.bits(exp["tophat"])[58:62, 210:250] == 0x7fc00000).all()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_a_constant_image(ctx, dtype):
    img = np.full((77, 270), 37, dtype)
    for radius in ((2, 2), (30, 12)):
        exp = R.all_ops_ref(img, radius)
        assert (exp["open"] == 37).all() and (exp["tophat"] == 0).all()
        check_all_ops(ctx, img, radius)


def test_a_small_call_after_a_large_one(ctx):
    """the workspace of the large call is the cache's when the small one takes its own"""
    big, small = R.make_image(700, 900, np.float32, 28), R.make_image(9, 11, np.float32, 29)
    check_all_ops(ctx, big, (40, 35), ("close", "tophat"))
    check_all_ops(ctx, small, (40, 35))
    check_all_ops(ctx, small, (1, 2))


def test_the_package_functions(ctx):
    import microaligner_amd as M
    from microaligner_amd.device import DeviceArray
    img = R.make_image(50, 70, np.uint16, 30)
    exp = R.all_ops_ref(img, (2, 4))
    for fn, op in ((M.grey_erode, "erode"), (M.grey_dilate, "dilate"), (M.grey_open, "open"), (M.grey_close, "close"),
                   (M.tophat, "tophat")):
        got = fn(img, (2, 4))
        assert isinstance(got, np.ndarray)
        same(got, exp[op], op)
    same(M.tophat(img, (2, 4), black=True), exp["blackhat"], "blackhat")
    d = M.grey_open(img, (2, 4), on_device=True)
    assert isinstance(d, DeviceArray)
    same(M.grey_dilate(d, 0), exp["open"], "a device array in")
    same(M.grey_erode(img, 3), R.morphology_ref(img, "erode", (3, 3)), "an int radius")
