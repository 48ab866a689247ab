"""-m gpu: Context.label_components, component_stats, remove_small_objects and fill_holes against the numpy statement of
tests/_components_ref.py, bit for bit: labels, count, areas, boxes and filtered images.  Everything is an integer and the
numbering is defined without a traversal order, so there is no tolerance anywhere.

csrc/components.hip labels tiles of T x T = 64 x 64 pixels in LDS and joins them across their borders; it has no other
change of path (one kernel sequence for every dtype, connectivity and size), so the shapes stand one below, at and one above
the tile in both axes, with one, two and more tiles along each, and the patterns put long chains, single atomic targets and
diagonal joins on the seams and the tile corners."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _components_ref as R  # noqa: E402

# The registry cases of the three entries (tests/_gpu_cases/components.py) register when that module is imported.  The
# package's own list of area modules does not name it, so this module imports it: it is collected before
# tests/test_gpu_stale_memory.py and tests/test_gpu_unaligned.py, which parametrise over the registry as it stands when they
# are imported.
pytest.register_assert_rewrite("_gpu_cases")
import _gpu_cases.components  # noqa: E402,F401

pytestmark = pytest.mark.gpu
T = R.T
I32_MAX = 2 ** 31 - 1
TOP = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 65535, np.dtype(np.int32): I32_MAX}


def same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype} {got.shape} against {exp.dtype} {exp.shape}"
    bad = got != exp
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:5].tolist()}"


def check_labels(ctx, img, connectivity, by_value=False, what=""):
    what = f"{what} {img.dtype} {img.shape} connectivity={connectivity} by_value={by_value}"
    exp, n = R.label_ref(img, connectivity, by_value)
    areas, boxes = R.stats_ref(exp, n)
    d_labels, count = ctx.label_components(ctx.components_asdevice(img), connectivity, by_value)
    assert count == n, f"{what}: {count} components against {n}"
    same(d_labels.numpy(), exp, f"labels {what}")
    d_areas, d_boxes = ctx.component_stats(d_labels, count)
    same(d_areas.numpy(), areas, f"areas {what}")
    same(d_boxes.numpy(), boxes, f"boxes {what}")
    return d_labels, n


def check_filters(ctx, img, connectivity, by_value=False, min_size=4, max_size=3, value=1, what=""):
    what = f"{what} {img.dtype} {img.shape} connectivity={connectivity}"
    d = ctx.components_asdevice(img)
    same(ctx.remove_small_objects(d, min_size, connectivity, by_value).numpy(), R.remove_small_ref(img, min_size, connectivity, by_value),
         f"remove_small_objects({min_size}, by_value={by_value}) {what}")
    if not by_value:
        for size in (None, max_size):
            same(ctx.fill_holes(d, size, connectivity, value).numpy(), R.fill_holes_ref(img, size, connectivity, value),
                 f"fill_holes({size}, value={value}) {what}")


def check_all(ctx, img, connectivity, what="", **kw):
    check_labels(ctx, img, connectivity, what=what)
    check_filters(ctx, img, connectivity, what=what, **kw)


def patterns(H, W):
    """the patterns every shape takes: (name, 0/1 mask)"""
    out = [("zeros", R.zeros(H, W)), ("ones", R.ones(H, W))]
    out += [(f"random {d}", R.random_mask(H, W, d, 100 + k)) for k, d in enumerate((0.3, 0.5, 0.593, 0.7))]
    out += [("checkerboard", R.checkerboard(H, W)), ("serpentine", R.serpentine(H, W)), ("spiral", R.spiral(H, W)),
            ("rings", R.rings(H, W))]
    return out


SHAPES = [(1, 1), (1, 300), (200, 1)] + [(h, w) for h in (T - 1, T, T + 1) for w in (T - 1, T, T + 1)] + \
         [(2 * T + 1, 3 * T + 1), (263, 301), (130, 70)]


@pytest.mark.parametrize("connectivity", (1, 2))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_patterns_at_the_shapes_around_the_tile(ctx, shape, connectivity):
    """the dtype goes round with the pattern and the shape, the foreground value between 1 and the dtype's largest"""
    for k, (name, mask) in enumerate(patterns(*shape)):
        dtype = R.DTYPES[(k + SHAPES.index(shape)) % 3]
        img = R.as_dtype(mask, dtype, top=k % 2 == 1)
        check_all(ctx, img, connectivity, what=name, value=TOP[np.dtype(dtype)] if k % 2 else 1)


@pytest.mark.parametrize("connectivity", (1, 2))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_dtype_on_every_pattern(ctx, dtype, connectivity):
    for name, mask in patterns(2 * T + 1, 3 * T + 1):
        check_all(ctx, R.as_dtype(mask, dtype), connectivity, what=name)
    # the largest values of the dtype as foreground and as the fill
    img = R.as_dtype(R.random_mask(70, 90, 0.6, 9), dtype, top=True)
    check_all(ctx, img, connectivity, what="largest value", value=TOP[np.dtype(dtype)])


@pytest.mark.parametrize("connectivity", (1, 2))
def test_joins_at_the_tile_corners_only(ctx, connectivity):
    """a diagonal line whose consecutive pixels meet only at the corner of four tiles: one component under 8 neighbours, one
    per pixel under 4"""
    for shape in ((2 * T + 1, 3 * T + 1), (T + 1, T + 1), (263, 301)):
        for name, mask in (("main diagonal", R.main_diagonal(*shape)), ("anti diagonal", R.anti_diagonal(*shape))):
            _, n = check_labels(ctx, mask, connectivity, what=name)
            assert n == (1 if connectivity == 2 else int(mask.sum()))
            check_filters(ctx, mask, connectivity, what=name, min_size=10)
            check_filters(ctx, 1 - mask, connectivity, what=f"{name}, inverted")
        both = R.main_diagonal(*shape) | R.anti_diagonal(*shape)
        check_all(ctx, both, connectivity, what="both diagonals")


@pytest.mark.parametrize("connectivity", (1, 2))
def test_components_whose_smallest_pixel_is_in_another_tile(ctx, connectivity):
    for shape in ((2 * T + 1, 3 * T + 1), (263, 301)):
        uj = R.u_and_j(*shape)
        _, n = check_labels(ctx, uj.astype(np.uint16), connectivity, what="U and J")
        assert n == 2
        check_filters(ctx, uj, connectivity, what="U and J", min_size=int(uj.sum()) // 2)
        check_all(ctx, uj[::-1].copy(), connectivity, what="U and J upside down")
        check_all(ctx, uj.T.copy(), connectivity, what="U and J transposed")


@pytest.mark.parametrize("connectivity", (1, 2))
def test_holes_that_touch_the_border_at_one_pixel(ctx, connectivity):
    for shape in ((40, 50), (T + 1, 2 * T), (263, 301)):
        b = R.border_holes(*shape)
        exp = R.fill_holes_ref(b, None, connectivity)
        assert np.count_nonzero(exp != b) == 3 * 12 + 1 + (4 * 4 if connectivity == 1 else 0)
        for dtype in R.DTYPES:
            check_filters(ctx, R.as_dtype(b, dtype), connectivity, what="border holes", max_size=4, value=TOP[np.dtype(dtype)])
        check_labels(ctx, 1 - b, connectivity, what="border holes, inverted")


@pytest.mark.parametrize("connectivity", (1, 2))
def test_sizes_at_the_thresholds(ctx, connectivity):
    """objects of exactly min_size - 1 and min_size pixels, holes of exactly max_size and max_size + 1"""
    for size, shape in ((1, (9, 20)), (12, (12, 40)), (70, (T + 5, 2 * T + 30))):
        blobs = R.sized_blobs(*shape, size)
        d = ctx.asdevice(blobs)
        for min_size in (size, size + 1, size + 2):
            exp = R.remove_small_ref(blobs, min_size, connectivity)
            assert np.count_nonzero(exp) == (2 * size + 1 if min_size == size else size + 1 if min_size == size + 1 else 0)
            same(ctx.remove_small_objects(d, min_size, connectivity).numpy(), exp, f"objects of {size} and {size + 1}, min_size {min_size}")
        holes = R.sized_blobs(*shape, size, 0, 1)
        d = ctx.asdevice(holes)
        for max_size in (size - 1, size, size + 1):
            exp = R.fill_holes_ref(holes, max_size, connectivity, 7)
            assert np.count_nonzero(exp == 7) == (0 if max_size < size else size if max_size == size else 2 * size + 1)
            same(ctx.fill_holes(d, max_size, connectivity, 7).numpy(), exp, f"holes of {size} and {size + 1}, max_size {max_size}")
    img = R.random_mask(70, 90, 0.5, 11)
    d = ctx.asdevice(img)
    for min_size in (0, 1):
        same(ctx.remove_small_objects(d, min_size, connectivity).numpy(), img, f"min_size {min_size}")
    for min_size in (img.size, img.size + 1, 2 ** 40):
        same(ctx.remove_small_objects(d, min_size, connectivity).numpy(), np.zeros_like(img), f"min_size {min_size}")
    same(ctx.remove_small_objects(ctx.asdevice(R.ones(70, 90)), 70 * 90, connectivity).numpy(), R.ones(70, 90), "the whole image")
    same(ctx.fill_holes(d, 0, connectivity).numpy(), img, "max_size 0")
    same(ctx.fill_holes(d, 2 ** 40, connectivity).numpy(), R.fill_holes_ref(img, None, connectivity), "max_size 2^40")


@pytest.mark.parametrize("connectivity", (1, 2))
def test_by_value(ctx, connectivity):
    rng = np.random.default_rng(12)
    for dtype in R.DTYPES:
        img = rng.integers(0, 4, (2 * T + 1, 3 * T + 1)).astype(dtype)
        check_labels(ctx, img, connectivity, True, what="values 0 .. 3")
        check_filters(ctx, img, connectivity, True, what="values 0 .. 3")
        check_all(ctx, img, connectivity, what="values 0 .. 3, not by value")
    two = np.zeros((T + 20, 2 * T + 20), np.uint16)
    two[3:T + 9, 4:T] = 7
    two[3:T + 9, T:T + 30] = 7               # equal values that touch along a tile border: one component
    two[T + 11:T + 17, 4:T] = 7
    two[T + 11:T + 17, T:T + 30] = 65535     # different values: two
    _, n = check_labels(ctx, two, connectivity, True, what="touching rectangles")
    assert n == 3
    _, n = check_labels(ctx, two, connectivity, False, what="touching rectangles")
    assert n == 2
    check_filters(ctx, two, connectivity, True, min_size=6 * 30 + 1, what="touching rectangles")
    ext = rng.choice(np.array([0, -5, I32_MAX, -2 ** 31, 1], np.int32), (T + 3, 2 * T + 5))
    check_labels(ctx, ext, connectivity, True, what="negative values and INT32_MAX")
    check_filters(ctx, ext, connectivity, True, what="negative values and INT32_MAX")
    check_all(ctx, ext, connectivity, what="negative values are foreground", value=I32_MAX)


@pytest.mark.parametrize("connectivity", (1, 2))
def test_labels_fed_back_in_come_back(ctx, connectivity):
    img = R.random_mask(2 * T + 1, 3 * T + 1, 0.55, 13)
    d_labels, n = check_labels(ctx, img, connectivity)
    again, m = ctx.label_components(d_labels, connectivity, True)
    assert m == n
    same(again.numpy(), d_labels.numpy(), "the labels of the labels")
    # a label image torn apart: the pieces of every label
    torn = d_labels.numpy().copy()
    torn[:, 3 * T // 2] = 0
    torn[T] = 0
    check_labels(ctx, torn, connectivity, True, what="torn labels")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_both_filters_in_place(ctx, dtype):
    img = R.as_dtype(R.random_mask(140, 300, 0.55, 14), dtype, top=True)
    for connectivity in (1, 2):
        work = ctx.components_asdevice(img).copy()
        out = ctx.remove_small_objects(work, 9, connectivity, out=work)
        assert out is work
        same(out.numpy(), R.remove_small_ref(img, 9, connectivity), "remove_small_objects in place")
        work = ctx.components_asdevice(img).copy()
        out = ctx.fill_holes(work, 5, connectivity, 3, out=work)
        assert out is work
        same(out.numpy(), R.fill_holes_ref(img, 5, connectivity, 3), "fill_holes in place")
        work = ctx.components_asdevice(img).copy()
        assert ctx.remove_small_objects(work, 1, connectivity, out=work) is work
        same(work.numpy(), img, "min_size 1 in place")
    d = ctx.components_asdevice(img)
    with pytest.raises(ValueError):
        ctx.remove_small_objects(d, 3, out=ctx.empty((140, 300), np.float32))
    with pytest.raises(ValueError):
        ctx.fill_holes(d, out=ctx.empty((140, 301), dtype))
    with pytest.raises(ValueError):
        ctx.label_components(d, out=ctx.empty((140, 300), np.uint16))
    if dtype == np.int32:
        with pytest.raises(ValueError):
            ctx.label_components(d, out=d)
    out = ctx.empty((140, 300), np.int32)
    labels, n = ctx.label_components(d, out=out)
    assert labels is out
    same(out.numpy(), R.label_ref(img)[0], "labels into out")


@functools.lru_cache(maxsize=None)
def large():
    """the larger image and its statement, made once: (mask, labels, n, areas, boxes)"""
    mask = R.random_mask(2049, 1031, 0.593, 15)
    mask[1000:1003] = 1                       # and a component through every tile column
    labels, n = R.label_ref(mask, 1)
    return (mask, labels, n) + R.stats_ref(labels, n)


def test_a_larger_image(ctx):
    mask, labels, n, areas, boxes = large()
    d_labels, count = ctx.label_components(ctx.asdevice(mask), 1)
    assert count == n
    same(d_labels.numpy(), labels, "labels")
    d_areas, d_boxes = ctx.component_stats(d_labels, count)
    same(d_areas.numpy(), areas, "areas")
    same(d_boxes.numpy(), boxes, "boxes")
    exp = mask.copy()
    exp[areas[labels] < 50] = 0
    same(ctx.remove_small_objects(ctx.asdevice(mask), 50).numpy(), exp, "remove_small_objects")
    ser = R.serpentine(2049, 1031).astype(np.uint16)
    d_labels, count = ctx.label_components(ctx.asdevice(ser), 1)
    assert count == 1
    same(d_labels.numpy(), ser.astype(np.int32), "the serpentine")
    one = ctx.fill_holes(ctx.asdevice(R.rings(2049, 1031)), None, 1).numpy()
    same(one, R.ones(2049, 1031), "the rings filled")


def test_a_small_call_after_a_large_one_and_the_same_call_twice(ctx):
    """the workspace of the large call is the cache's when the small one takes its own; two runs give the same bits"""
    mask = large()[0]
    big = ctx.asdevice(mask)
    first = ctx.label_components(big, 2)
    second = ctx.label_components(big, 2)
    assert first[1] == second[1]
    same(first[0].numpy(), second[0].numpy(), "the same call twice")
    same(ctx.fill_holes(big, 30, 2).numpy(), ctx.fill_holes(big, 30, 2).numpy(), "the same filter twice")
    for shape in ((9, 11), (T + 1, T - 1)):
        check_all(ctx, R.random_mask(*shape, 0.5, 16), 1, what="after a large call")
        check_all(ctx, R.random_mask(*shape, 0.5, 17).astype(np.int32), 2, what="after a large call")


def test_the_package_functions(ctx):
    import microaligner_amd as M
    from microaligner_amd.device import DeviceArray
    img = R.random_mask(70, 150, 0.55, 18)
    for connectivity in (1, 2):
        exp, n = R.label_ref(img, connectivity)
        got = M.label_components(img, connectivity)
        assert isinstance(got, np.ndarray)
        same(got, exp, "labels")
        same(M.label_components(img.astype(bool), connectivity), exp, "a bool mask")
        got, info = M.label_components(img * np.uint8(255), connectivity, return_info=True)
        assert isinstance(info, M.ComponentInfo) and info.count == n
        areas, boxes = R.stats_ref(exp, n)
        same(got, exp, "labels with info")
        same(info.areas, areas, "areas")
        same(info.bboxes, boxes, "boxes")
        same(M.remove_small_objects(img, 7, connectivity), R.remove_small_ref(img, 7, connectivity), "remove_small_objects")
        same(M.remove_small_objects(img.astype(bool), 7, connectivity), R.remove_small_ref(img, 7, connectivity), "on a bool mask")
        same(M.fill_holes(img, None, connectivity), R.fill_holes_ref(img, None, connectivity), "fill_holes")
        same(M.fill_holes(img, 6, connectivity, 200), R.fill_holes_ref(img, 6, connectivity, 200), "fill_holes up to a size")
    d = M.label_components(img, on_device=True)
    assert isinstance(d, DeviceArray) and d.dtype == np.int32
    pieces, info = M.label_components(d, by_value=True, on_device=True, return_info=True)
    assert isinstance(pieces, DeviceArray) and isinstance(info.areas, np.ndarray)
    same(pieces.numpy(), R.label_ref(img)[0], "a device array in")
    kept = M.remove_small_objects(d, 7, by_value=True)
    same(kept, R.remove_small_ref(R.label_ref(img)[0], 7, 1, True), "labels filtered by value keep their values")
    empty, info = M.label_components(np.zeros((5, 6), np.uint16), return_info=True)
    assert info.count == 0 and info.areas.tolist() == [30] and info.bboxes.tolist() == [[0, 0, 0, 0]] and not empty.any()


def test_stats_of_labels_that_are_not_connected_or_absent(ctx):
    """ma_cc_stats takes any label image: pieces of one value add up, a value no pixel has gives zeros, values outside
    0 .. n take no part"""
    rng = np.random.default_rng(19)
    labels = rng.integers(-1, 9, (T + 7, 2 * T + 9)).astype(np.int32)
    labels[labels == 4] = 0
    for n in (7, 12):
        areas, boxes = R.stats_ref(labels, n)
        d_areas, d_boxes = ctx.component_stats(ctx.components_asdevice(labels), n)
        same(d_areas.numpy(), areas, f"areas n={n}")
        same(d_boxes.numpy(), boxes, f"boxes n={n}")
        assert areas[4] == 0 and not boxes[4].any()
