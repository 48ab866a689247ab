"""The connected components without a GPU (include/microaligner_components.h): the numpy statement of
tests/_components_ref.py against scipy.ndimage (label, find_objects, sum, binary_fill_holes) and the identities of the two
filters, then the refusals of the Python functions and of the C entries, which need no device, and the agreement of header,
library and bindings."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _components_ref as R  # noqa: E402

# the registry cases of ma_cc_label, ma_cc_stats and ma_cc_filter register when their module is imported; the package's own
# list does not name it
pytest.register_assert_rewrite("_gpu_cases")
import _gpu_cases as G  # noqa: E402
import _gpu_cases.components  # noqa: E402,F401

ndi = pytest.importorskip("scipy.ndimage")
T = R.T
H0, W0 = 2 * T + 1, 3 * T + 1

PATTERNS = {
    "zeros": lambda: R.zeros(40, 50),
    "ones": lambda: R.ones(40, 50),
    "random 0.3": lambda: R.random_mask(H0, W0, 0.3, 1),
    "random 0.5": lambda: R.random_mask(H0, W0, 0.5, 2),
    "random 0.593": lambda: R.random_mask(H0, W0, 0.593, 3),
    "random 0.7": lambda: R.random_mask(H0, W0, 0.7, 4),
    "checkerboard": lambda: R.checkerboard(33, 47),
    "serpentine": lambda: R.serpentine(H0, W0),
    "spiral": lambda: R.spiral(70, 91),
    "rings": lambda: R.rings(70, 91),
    "main diagonal": lambda: R.main_diagonal(H0, W0),
    "anti diagonal": lambda: R.anti_diagonal(H0, W0),
    "U and J": lambda: R.u_and_j(H0, W0),
    "border holes": lambda: R.border_holes(40, 50),
    "one pixel": lambda: R.ones(1, 1),
    "one row": lambda: R.random_mask(1, 300, 0.5, 5),
    "one column": lambda: R.random_mask(200, 1, 0.5, 6),
}


def structure(connectivity):
    return ndi.generate_binary_structure(2, connectivity)


def same(got, exp):
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("connectivity", (1, 2))
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_labels_areas_and_boxes_are_scipys(name, connectivity):
    img = PATTERNS[name]()
    labels, n = R.label_ref(img, connectivity)
    exp, en = ndi.label(img != 0, structure(connectivity))
    assert n == en and labels.dtype == np.int32
    same(labels, exp.astype(np.int32))
    areas, boxes = R.stats_ref(labels, n)
    assert areas.dtype == np.int64 and areas.shape == (n + 1,) and boxes.dtype == np.int32 and boxes.shape == (n + 1, 4)
    assert areas[0] == np.count_nonzero(img == 0) and not boxes[0].any()
    if n:
        assert np.array_equal(areas[1:], ndi.sum(np.ones_like(img, np.int64), exp, np.arange(1, n + 1)).astype(np.int64))
        objects = ndi.find_objects(exp)
        assert np.array_equal(boxes[1:], [[s[0].start, s[1].start, s[0].stop, s[1].stop] for s in objects])


def test_the_patterns_are_what_their_names_say():
    s = R.serpentine(H0, W0)
    assert R.label_ref(s, 1)[1] == 1 and s.any(axis=1).all() and s.sum() == (H0 + 1) // 2 * W0 + H0 // 2
    sp = R.spiral(70, 91)
    assert R.label_ref(sp, 1)[1] == 1 and R.label_ref(sp == 0, 1)[1] == 1 and sp.sum() > 70 * 91 // 3
    assert R.label_ref(R.rings(70, 91), 2)[1] == 18 and R.label_ref(R.rings(70, 91) == 0, 2)[1] == 17
    c = R.checkerboard(33, 47)
    assert R.label_ref(c, 1)[1] == c.sum() and R.label_ref(c, 2)[1] == 1
    for d, pair in ((R.main_diagonal(H0, W0), ((T - 1, T - 1), (T, T))), (R.anti_diagonal(H0, W0), ((T - 1, T), (T, T - 1)))):
        assert all(d[p] for p in pair)
        assert R.label_ref(d, 2)[1] == 1 and R.label_ref(d, 1)[1] == d.sum()
    uj = R.u_and_j(H0, W0)
    labels, n = R.label_ref(uj, 2)
    assert n == 2
    for k in (1, 2):                      # the smallest pixel lies in another tile than most of the component
        ys, xs = np.nonzero(labels == k)
        tiles = (ys // T) * 8 + xs // T
        assert np.bincount(tiles).argmax() != tiles[0]
    b = R.border_holes(40, 50)
    assert np.count_nonzero(R.fill_holes_ref(b, None, 1) != b) == 3 * 12 + 1 + 4 * 4
    assert np.count_nonzero(R.fill_holes_ref(b, None, 2) != b) == 3 * 12 + 1
    for size in (1, 5, 12):
        blobs = R.sized_blobs(12, 40, size)
        assert sorted(np.bincount(R.label_ref(blobs, 1)[0].ravel())[1:]) == [size, size + 1]


def label_by_value_scipy(img, connectivity):
    """every distinct value labelled on its own by scipy, the components renumbered by their first pixel"""
    first, pieces = [], []
    for v in np.unique(img):
        if v == 0:
            continue
        lab, n = ndi.label(img == v, structure(connectivity))
        for k in range(1, n + 1):
            m = lab == k
            first.append(int(np.flatnonzero(m.ravel())[0]))
            pieces.append(m)
    out = np.zeros(img.shape, np.int32)
    for k, i in enumerate(np.argsort(first), 1):
        out[pieces[i]] = k
    return out, len(pieces)


def by_value_images():
    rng = np.random.default_rng(7)
    yield rng.integers(0, 4, (70, 90)).astype(np.uint8)
    two = np.zeros((20, 30), np.uint16)
    two[3:9, 4:12] = 7
    two[3:9, 12:20] = 7          # equal values: one component
    two[11:17, 4:12] = 7
    two[11:17, 12:20] = 65535    # different values: two
    yield two
    ext = rng.choice(np.array([0, -5, 2 ** 31 - 1, 1], np.int32), (40, 50))
    yield ext
    yield R.label_ref(R.random_mask(50, 60, 0.5, 8), 1)[0]


@pytest.mark.parametrize("connectivity", (1, 2))
def test_by_value_is_scipy_value_by_value(connectivity):
    for img in by_value_images():
        got, n = R.label_ref(img, connectivity, True)
        exp, en = label_by_value_scipy(img, connectivity)
        assert n == en
        same(got, exp)
    # the labels of an image, labelled by value, are themselves
    lab, n = R.label_ref(R.random_mask(50, 60, 0.5, 8), connectivity)
    again, m = R.label_ref(lab, connectivity, True)
    assert m == n
    same(again, lab)


@pytest.mark.parametrize("connectivity", (1, 2))
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_fill_holes_is_scipys(name, connectivity):
    img = PATTERNS[name]()
    got = R.fill_holes_ref(img, None, connectivity)
    same(got, ndi.binary_fill_holes(img != 0, structure(connectivity)).astype(np.uint8))
    same(R.fill_holes_ref(got, None, connectivity), got)                                  # idempotent
    back, n = R.label_ref(got == 0, connectivity)
    rim = np.unique(np.concatenate([back[0], back[-1], back[:, 0], back[:, -1]]))
    assert set(range(1, n + 1)) <= set(rim.tolist())               # no background component is left that misses the border


@pytest.mark.parametrize("connectivity", (1, 2))
@pytest.mark.parametrize("name", ["random 0.3", "random 0.5", "random 0.593", "rings", "U and J", "border holes"])
def test_remove_small_objects(name, connectivity):
    img = PATTERNS[name]()
    labels, n = ndi.label(img != 0, structure(connectivity))
    for min_size in (0, 1, 2, 5, 40):
        got = R.remove_small_ref(img, min_size, connectivity)
        try:
            from skimage.morphology import remove_small_objects
            keep = remove_small_objects(img != 0, min_size, connectivity=connectivity)
        except ImportError:
            keep = (np.bincount(labels.ravel())[labels] >= min_size) & (labels > 0)
        same(got, np.where(keep, img, 0).astype(img.dtype))
        if min_size <= 1:
            same(got, img)
        # the labels of the image and of what is left agree up to renumbering on the kept pixels
        mine, _ = R.label_ref(img, connectivity)
        left, _ = R.label_ref(got, connectivity)
        kept = got != 0
        pairs = np.unique(np.stack([mine[kept], left[kept]], axis=1), axis=0)
        assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])) == R.label_ref(got, connectivity)[1]
    assert not R.remove_small_ref(img, img.size + 1, connectivity).any()


def test_sizes_at_the_threshold():
    blobs = R.sized_blobs(12, 40, 12)
    assert sorted(np.bincount(R.label_ref(R.remove_small_ref(blobs, 13), 1)[0].ravel())[1:]) == [13]
    same(R.remove_small_ref(blobs, 12), blobs)
    holes = R.sized_blobs(12, 40, 12, 0, 1)
    filled = R.fill_holes_ref(holes, 12, 1, 9)
    assert np.count_nonzero(filled == 9) == 12 and np.count_nonzero(filled == 0) == 13
    assert np.count_nonzero(R.fill_holes_ref(holes, 13, 1, 9) == 0) == 0
    same(R.fill_holes_ref(holes, 11, 1, 9), holes)
    same(R.fill_holes_ref(holes, 0, 1, 9), holes)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def Huge(shape, dtype=np.uint8):
    """a device array of a size nobody allocates here: the checks look at its shape and dtype only"""
    from microaligner_amd.device import DeviceArray
    d = DeviceArray.__new__(DeviceArray)
    d.ctx, d.shape, d.dtype, d.ptr = None, tuple(shape), np.dtype(dtype), None
    return d


def test_python_refusals_need_no_context(monkeypatch):
    import microaligner_amd as M
    from microaligner_amd import device
    monkeypatch.setattr(device, "get_context", lambda *a, **k: pytest.fail("a context was made"))
    img = np.zeros((8, 9), np.uint8)
    calls = (lambda a, **k: M.label_components(a, **k), lambda a, **k: M.remove_small_objects(a, 3, **k),
             lambda a, **k: M.fill_holes(a, **k))
    for fn in calls:
        for bad in (np.zeros((8, 9), np.float32), np.zeros((8, 9), np.int16), np.zeros((8, 9), np.int64), np.zeros((8, 9), np.uint32),
                    np.zeros((8,), np.uint8), np.zeros((2, 8, 9), np.uint8), np.zeros((0, 9), np.uint8), np.zeros((8, 0), np.int32),
                    [[1, 2]], None, Huge((1 << 16, 1 << 15)), Huge((46341, 46341), np.int32), Huge(((1 << 24) + 1, 1))):
            with pytest.raises(ValueError):
                fn(bad)
        for bad in (0, 3, 8, True, 1.0, "1", None):
            with pytest.raises(ValueError):
                fn(img, connectivity=bad)
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError):
                fn(img, on_device=bad)
    for bad in (1, 0, None):
        with pytest.raises(ValueError):
            M.label_components(img, by_value=bad)
        with pytest.raises(ValueError):
            M.remove_small_objects(img, 3, by_value=bad)
        with pytest.raises(ValueError):
            M.label_components(img, return_info=bad)
    for bad in (-1, 1.0, True, "3", None, np.float32(2)):
        with pytest.raises(ValueError):
            M.remove_small_objects(img, bad)
    for bad in (-1, 1.0, True, "3"):
        with pytest.raises(ValueError):
            M.fill_holes(img, max_size=bad)
    for arr, values in ((img, (0, 256, -1, 1.0, True, None)), (np.zeros((8, 9), np.uint16), (0, 65536)),
                        (np.zeros((8, 9), np.int32), (0, 2 ** 31, -1)), (np.zeros((8, 9), bool), (256,))):
        for bad in values:
            with pytest.raises(ValueError):
                M.fill_holes(arr, value=bad)
    L = device.L
    assert device.components_params(np.zeros((3, 4), bool), 2, True) == (3, 4, L.MA_U8, 3)
    assert device.components_params(Huge((46340, 46341), np.int32)) == (46340, 46341, L.MA_CC_I32, 0)
    assert device.components_params(Huge((1, 1 << 24), np.uint16), np.int64(1), np.bool_(False)) == (1, 1 << 24, L.MA_U16, 0)
    assert device.remove_small_params(img, np.int64(2 ** 40), 2) == (8, 9, L.MA_U8, 1, 2 ** 40)
    assert device.fill_holes_params(img, None, 1, 255) == (8, 9, L.MA_U8, 4, 2 ** 31 - 1, 255)
    assert device.fill_holes_params(np.zeros((8, 9), np.int32), 2 ** 40, 2, 2 ** 31 - 1) == (8, 9, L.MA_CC_I32, 5, 2 ** 31 - 1, 2 ** 31 - 1)


def test_c_refusals_need_no_device():
    from microaligner_amd import _lib as L
    lib = L.load()
    ctx, p, q, r = 1 << 30, 2 << 30, 3 << 30, 4 << 30          # never dereferenced: every call below is refused first
    n = C.c_longlong(-9)
    label, stats, filt = lib.ma_cc_label, lib.ma_cc_stats, lib.ma_cc_filter
    M = L.MA_CC_MAX_PIXELS
    assert label(None, p, L.MA_U8, 8, 8, 0, q, C.byref(n)) == L.MA_EINVAL
    assert b"invalid argument" in lib.ma_last_error()
    assert label(ctx, None, L.MA_U8, 8, 8, 0, q, C.byref(n)) == L.MA_EINVAL
    assert label(ctx, p, L.MA_U8, 8, 8, 0, None, C.byref(n)) == L.MA_EINVAL
    assert label(ctx, p, L.MA_U8, 8, 8, 0, q, None) == L.MA_EINVAL
    assert stats(None, p, 8, 8, 1, q, r) == stats(ctx, None, 8, 8, 1, q, r) == L.MA_EINVAL
    assert stats(ctx, p, 8, 8, 1, None, r) == stats(ctx, p, 8, 8, 1, q, None) == L.MA_EINVAL
    assert filt(None, p, L.MA_U8, 8, 8, 0, 2, M, 0, q) == filt(ctx, None, L.MA_U8, 8, 8, 0, 2, M, 0, q) == L.MA_EINVAL
    assert filt(ctx, p, L.MA_U8, 8, 8, 0, 2, M, 0, None) == L.MA_EINVAL
    for dtype in (-1, L.MA_F32, 4):
        assert label(ctx, p, dtype, 8, 8, 0, q, C.byref(n)) == L.MA_EINVAL
        assert b"dtype" in lib.ma_last_error()
        assert filt(ctx, p, dtype, 8, 8, 0, 2, M, 0, q) == L.MA_EINVAL
    sides = ((0, 8), (8, 0), (-1, 8), ((1 << 24) + 1, 1), (1, (1 << 24) + 1), (1 << 16, 1 << 15), (46341, 46341), (1 << 24, 1 << 24))
    for H, W in sides:
        assert label(ctx, p, L.MA_U8, H, W, 0, q, C.byref(n)) == L.MA_EINVAL
        assert stats(ctx, p, H, W, 1, q, r) == L.MA_EINVAL
        assert filt(ctx, p, L.MA_U16, H, W, 0, 2, M, 0, q) == L.MA_EINVAL
    assert b"too large" in lib.ma_last_error()
    for flags in (-1, 4, 8, 7 + 8):
        assert label(ctx, p, L.MA_U8, 8, 8, flags, q, C.byref(n)) == L.MA_EINVAL
    for flags in (-1, 8, L.MA_CC_HOLES | L.MA_CC_BY_VALUE, 7):
        assert filt(ctx, p, L.MA_U8, 8, 8, flags, 0, M, 1, q) == L.MA_EINVAL
    assert label(ctx, p, L.MA_CC_I32, 8, 8, 0, p, C.byref(n)) == L.MA_EINVAL              # labels over src
    assert label(ctx, p, L.MA_CC_I32, 8, 8, 0, p + 4 * 63, C.byref(n)) == L.MA_EINVAL
    assert b"overlap" in lib.ma_last_error()
    for bad in (-1, M):
        assert stats(ctx, p, 8, 8, bad, q, r) == L.MA_EINVAL
    for lo, hi in ((-1, M), (0, -1), (M + 1, M), (0, M + 1)):
        assert filt(ctx, p, L.MA_U8, 8, 8, 0, lo, hi, 0, q) == L.MA_EINVAL
    for dtype, values in ((L.MA_U8, (0, 256, -1)), (L.MA_U16, (0, 65536)), (L.MA_CC_I32, (0, 2 ** 31, -1))):
        for v in values:
            assert filt(ctx, p, dtype, 8, 8, L.MA_CC_HOLES, 0, M, v, q) == L.MA_EINVAL
            assert b"value" in lib.ma_last_error()
    assert n.value == -9


def test_header_library_and_bindings_agree():
    import re
    from microaligner_amd import _lib as L, build
    from _measured_path import HASH
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "microaligner_components.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["ma_cc_filter", "ma_cc_label", "ma_cc_stats"]
    assert sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", code))) == names == sorted(L.COMPONENTS_SIGNATURES)
    vals = {k: int(v) for k, v in re.findall(r"\b(MA_CC_[A-Z0-9_]+)\s*=\s*(\d+)", code)}
    vals.update({k: int(v) for k, v in re.findall(r"#define\s+(MA_CC_[A-Z0-9_]+)\s+(\d+)", code)})
    assert len(vals) == 6
    for name, v in vals.items():
        assert getattr(L, name) == v, name
    assert L.MA_CC_I32 not in (L.MA_U8, L.MA_U16, L.MA_F32) and L.MA_CC_TILE == R.T
    ll, vp, i = C.c_longlong, C.c_void_p, C.c_int
    assert L.COMPONENTS_SIGNATURES["ma_cc_label"] == (i, [vp, vp, i, i, i, i, vp, C.POINTER(ll)])
    assert L.COMPONENTS_SIGNATURES["ma_cc_stats"] == (i, [vp, vp, i, i, ll, vp, vp])
    assert L.COMPONENTS_SIGNATURES["ma_cc_filter"] == (i, [vp, vp, i, i, i, i, ll, ll, ll, vp])
    lib = L.load()
    assert all(hasattr(lib, name) for name in names)
    # off the measured path: the hash is the one the tests of the measured path hold, and the library's
    assert "components.hip" in build.SOURCES and build.source_hash() == HASH == L.source_hash()
    assert [os.path.basename(h) for h in build.SOURCE_HEADERS["components.hip"]] == ["microaligner_components.h"]
    src = open(os.path.join(build.CSRC, "components.hip")).read()
    assert "MA_REQUIRE_ALIGNED" not in src
    import microaligner_amd as M
    assert {"label_components", "remove_small_objects", "fill_holes", "ComponentInfo"} <= set(M.__all__)


def test_the_registry_holds_the_entries():
    """with the cases' module imported (here and by tests/test_gpu_components.py, before the two suites that run the registry
    are collected) the completeness check of tests/test_debug_fill.py holds for the new entries"""
    for entry in ("ma_cc_label", "ma_cc_stats", "ma_cc_filter"):
        assert entry in G.declared_entries() and entry not in G.EXEMPT
    assert sum("ma_cc_filter" in c.entries for c in G.CASES) == 2
    assert sum("ma_cc_label" in c.entries for c in G.CASES) == 1
