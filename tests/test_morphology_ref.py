"""The flat grey morphology without a GPU (include/microaligner_morphology.h): the numpy statement of tests/_morph_ref.py
against scipy.ndimage and against a brute-force loop, the exact identities the header lists, the two properties the functions
are there for (a mask loses exactly the rectangles that do not hold the element; a top-hat gives small spots back exactly),
one described usefulness figure, and every refusal of the Python layers and of the C entry that needs no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _morph_ref as R  # noqa: E402

# the registry cases of ma_morphology register when their module is imported; the package's own list does not name it
pytest.register_assert_rewrite("_gpu_cases")
import _gpu_cases as G  # noqa: E402
import _gpu_cases.morphology  # noqa: E402,F401

INT_DTYPES = (np.uint8, np.uint16)
ids = lambda d: np.dtype(d).name  # noqa: E731


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    bad = R.bits(a) != R.bits(b)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:5].tolist()}"


# ---- against scipy and brute force ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [(0, 0), (0, 3), (3, 0), (1, 1), (2, 5), (7, 7), (20, 9)], ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_the_statement_is_scipy_with_a_replicated_border(dtype, radius):
    ndi = pytest.importorskip("scipy.ndimage")
    img = R.make_image(37, 53, dtype, 1, specials=np.dtype(dtype) != np.float32)      # finite floats only
    size = (2 * radius[0] + 1, 2 * radius[1] + 1)
    same(R.morphology_ref(img, "erode", radius), ndi.minimum_filter(img, size=size, mode="nearest"))
    same(R.morphology_ref(img, "dilate", radius), ndi.maximum_filter(img, size=size, mode="nearest"))
    same(R.morphology_ref(img, "open", radius), ndi.grey_opening(img, size=size, mode="nearest"))
    same(R.morphology_ref(img, "close", radius), ndi.grey_closing(img, size=size, mode="nearest"))
    same(R.morphology_ref(img, "tophat", radius), ndi.white_tophat(img, size=size, mode="nearest"))
    same(R.morphology_ref(img, "blackhat", radius), ndi.black_tophat(img, size=size, mode="nearest"))


@pytest.mark.parametrize("shape, radius", [((9, 13), (1, 2)), ((12, 10), (3, 3)), ((5, 7), (9, 11)), ((1, 6), (2, 2)),
                                           ((6, 1), (2, 0)), ((1, 1), (4, 4))], ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_the_statement_is_the_brute_force_window(dtype, shape, radius):
    """borders, images smaller than the window, and for float32 NaNs of both signs, +-Inf, +-0 and denormals"""
    img = R.make_image(*shape, dtype, 2)
    if np.dtype(dtype) == np.float32:
        img.flat[::3] = R.SPECIALS[np.arange(img.size)[::3] % R.SPECIALS.size]
    for maximum in (False, True):
        same(R.primitive(img, radius, maximum), R.brute(img, radius, maximum))
    # open and close are the primitive applied twice, NaN rule included
    same(R.morphology_ref(img, "open", radius), R.brute(R.brute(img, radius, False), radius, True))
    same(R.morphology_ref(img, "close", radius), R.brute(R.brute(img, radius, True), radius, False))


def test_float_order_nan_rule_and_hats():
    f = lambda *bits: np.array(bits, np.uint32).view(np.float32).reshape(1, -1)  # noqa: E731
    row = f(0x80000000, 0x00000000, 0x7fc00001, 0x00000001, 0x80000001)         # -0, +0, NaN, +denormal, -denormal
    same(R.morphology_ref(row, "erode", (0, 1)), f(0x80000000, 0x80000000, 0x00000000, 0x80000001, 0x80000001))
    same(R.morphology_ref(row, "dilate", (0, 1)), f(0x00000000, 0x00000000, 0x00000001, 0x00000001, 0x00000001))
    nans = f(0xffc00000, 0x7f800001, 0xffffffff)
    for op in R.OPS:
        same(R.morphology_ref(nans, op, 1), f(0x7fc00000, 0x7fc00000, 0x7fc00000))                   # all-NaN windows
        same(R.morphology_ref(nans, op, 0), f(0x7fc00000, 0x7fc00000, 0x7fc00000))
    inf = f(0x7f800000, 0x7f800000, 0x7f800000, 0x3f800000, 0xff800000)
    # open of a row of +Inf is +Inf: Inf - Inf is the NaN of bits 0x7fc00000, not the machine's
    same(R.morphology_ref(inf, "tophat", (0, 1))[:, :2], f(0x7fc00000, 0x7fc00000))
    same(R.morphology_ref(inf, "erode", (0, 1)), f(0x7f800000, 0x7f800000, 0x3f800000, 0xff800000, 0xff800000))
    big = f(0x7f7fffff, 0xff7fffff, 0x7f7fffff)
    same(R.morphology_ref(big, "tophat", (0, 1)), f(0x7f800000, 0x00000000, 0x7f800000))              # FLT_MAX - -FLT_MAX


# ---- exact properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [(1, 1), (2, 5), (9, 4)], ids=str)
@pytest.mark.parametrize("dtype", INT_DTYPES, ids=ids)
def test_exact_identities(dtype, radius):
    x = R.make_image(61, 83, dtype, 3)
    o, c = R.morphology_ref(x, "open", radius), R.morphology_ref(x, "close", radius)
    assert (o <= x).all() and (x <= c).all()
    same(R.morphology_ref(o, "open", radius), o)
    same(R.morphology_ref(c, "close", radius), c)
    M = np.iinfo(dtype).max
    same(R.morphology_ref(x, "dilate", radius), (M - R.morphology_ref((M - x).astype(dtype), "erode", radius)).astype(dtype))
    same(R.morphology_ref(x, "tophat", radius), (x - o).astype(dtype))
    same(R.morphology_ref(x, "blackhat", radius), (c - x).astype(dtype))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_radii_add(dtype):
    """erode(r1) then erode(r2) is erode(r1 + r2) with cut windows, NaN rule included: what lets a pass split a radius"""
    x = R.make_image(47, 58, dtype, 4)
    for r1, r2 in (((1, 2), (3, 1)), ((5, 0), (0, 7)), ((30, 40), (25, 30))):
        total = (r1[0] + r2[0], r1[1] + r2[1])
        for maximum in (False, True):
            same(R.primitive(R.primitive(x, r1, maximum), r2, maximum), R.primitive(x, total, maximum))


# ---- the two usefulness properties ----------------------------------------------------------------------------------------
def test_open_deletes_exactly_the_rectangles_that_do_not_hold_the_element():
    rng = np.random.default_rng(5)
    H, W, ry, rx = 150, 200, 3, 5
    mask = np.zeros((H, W), np.uint8)
    taken = np.zeros((H, W), bool)          # rectangles grown by one pixel: no two touch, not even at a corner
    rects = []
    for _ in range(400):
        h, w = int(rng.integers(1, 16)), int(rng.integers(1, 24))
        y, x = int(rng.integers(1, H - h - 1)), int(rng.integers(1, W - w - 1))
        if taken[y - 1:y + h + 1, x - 1:x + w + 1].any():
            continue
        taken[y - 1:y + h + 1, x - 1:x + w + 1] = True
        mask[y:y + h, x:x + w] = 255
        rects.append((y, x, h, w))
    kept = [r for r in rects if r[2] >= 2 * ry + 1 and r[3] >= 2 * rx + 1]
    assert len(rects) > 30 and 3 < len(kept) < len(rects) - 3
    exp = np.zeros_like(mask)
    for y, x, h, w in kept:
        exp[y:y + h, x:x + w] = 255
    same(R.morphology_ref(mask, "open", (ry, rx)), exp)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=ids)
def test_tophat_gives_small_spots_on_a_constant_back_exactly(dtype):
    rng = np.random.default_rng(6)
    H, W, r = 120, 140, 6
    spots = np.zeros((H, W), dtype)
    taken = np.zeros((H, W), bool)          # spots grown by one pixel: no two touch, so no two make up a larger one
    for _ in range(40):
        h, w = int(rng.integers(1, 2 * r + 1)), int(rng.integers(1, 2 * r + 1))        # smaller than the element on both axes
        y, x = int(rng.integers(r + 1, H - h - r - 1)), int(rng.integers(r + 1, W - w - r - 1))
        if taken[y - 1:y + h + 1, x - 1:x + w + 1].any():
            continue
        taken[y - 1:y + h + 1, x - 1:x + w + 1] = True
        spots[y:y + h, x:x + w] = rng.integers(1, 100, (h, w)).astype(dtype)
    assert (spots > 0).sum() > 300
    img = (spots + dtype(50)).astype(dtype)
    same(R.morphology_ref(img, "tophat", r), spots)


def synthetic_background_case(seed=7, n=256, r=15):
    """a smooth additive background, discs of radius up to 6 and noise: (image, background, discs)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    bg = 2000.0 + 1500.0 * np.sin(yy / 90.0) * np.cos(xx / 70.0) + 4.0 * xx
    discs = np.zeros((n, n))
    for _ in range(60):
        cy, cx, rad = rng.uniform(10, n - 10), rng.uniform(10, n - 10), rng.uniform(2, 6)
        discs[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad ** 2] = rng.uniform(800, 3000)
    img = np.clip(bg + discs + rng.normal(0, 20, (n, n)), 0, 65535).astype(np.uint16)
    return img, bg, discs


def test_usefulness_figure_is_reported(capsys):
    """a description, not a threshold: the residual background away from the discs before and after tophat(r = 15), seed 7"""
    img, bg, discs = synthetic_background_case()
    th = R.morphology_ref(img, "tophat", 15)
    off = discs == 0
    before = float(np.std(img[off].astype(np.float64)))
    after = float(np.std(th[off].astype(np.float64)))
    on = discs > 0
    kept = float(np.mean(th[on].astype(np.float64)) / np.mean(discs[on]))
    with capsys.disabled():
        print(f"\ntophat r=15, seed 7, 256x256 uint16: background s.d. off the discs {before:.1f} -> {after:.1f} grey levels; "
              f"mean disc height kept {kept:.3f}")
    assert th.dtype == np.uint16 and th.shape == img.shape


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_context(monkeypatch):
    import microaligner_amd as M
    from microaligner_amd import device
    monkeypatch.setattr(device, "get_context", lambda *a, **k: pytest.fail("a context was made"))
    img = np.zeros((8, 9), np.uint8)
    fns = (M.grey_erode, M.grey_dilate, M.grey_open, M.grey_close, M.tophat)
    for fn in fns:
        for bad in (np.zeros((8, 9), np.int16), np.zeros((8, 9), np.float64), np.zeros((8, 9), bool), np.zeros((8,), np.uint8),
                    np.zeros((2, 8, 9), np.uint8), np.zeros((0, 9), np.uint8), np.zeros((8, 0), np.float32), [[1, 2]], None):
            with pytest.raises(ValueError):
                fn(bad, 1)
        for bad in (True, 1.0, -1, 256, (1,), (1, 2, 3), (1, -1), (256, 0), (1.0, 1), (True, 1), "3", None, np.float32(2)):
            with pytest.raises(ValueError):
                fn(img, bad)
        with pytest.raises(ValueError):
            fn(img, 1, on_device=1)
    with pytest.raises(ValueError):
        M.tophat(img, 1, black=1)
    with pytest.raises(ValueError):
        device.morphology_params(img, "gradient", 1)
    assert device.morphology_params(img, "tophat", np.int64(255)) == (8, 9, 0, 4, 255, 255)
    assert device.morphology_params(np.zeros((3, 4), np.float32), "erode", [0, 7]) == (3, 4, 2, 0, 0, 7)
    assert set(device.MORPH_OPS) == set(R.OPS)


def test_c_refusals_need_no_device():
    from microaligner_amd import _lib as L
    lib = L.load()
    f = lib.ma_morphology
    ctx, p, q = 1 << 20, 2 << 20, 3 << 20          # never dereferenced: every call below is refused first
    assert f(None, p, L.MA_U8, 8, 8, L.MA_MORPH_ERODE, 1, 1, q) == L.MA_EINVAL
    assert b"invalid argument" in lib.ma_last_error()
    assert f(ctx, None, L.MA_U8, 8, 8, L.MA_MORPH_ERODE, 1, 1, q) == L.MA_EINVAL
    assert f(ctx, p, L.MA_U8, 8, 8, L.MA_MORPH_ERODE, 1, 1, None) == L.MA_EINVAL
    for dtype in (-1, 3):
        assert f(ctx, p, dtype, 8, 8, L.MA_MORPH_ERODE, 1, 1, q) == L.MA_EINVAL
    for op in (-1, 6):
        assert f(ctx, p, L.MA_U8, 8, 8, op, 1, 1, q) == L.MA_EINVAL
    for H, W in ((0, 8), (8, 0), (-1, 8), ((1 << 24) + 1, 8), (8, (1 << 24) + 1)):
        assert f(ctx, p, L.MA_U16, H, W, L.MA_MORPH_OPEN, 1, 1, q) == L.MA_EINVAL
    for ry, rx in ((-1, 0), (0, -1), (256, 0), (0, 256)):
        assert f(ctx, p, L.MA_F32, 8, 8, L.MA_MORPH_TOPHAT, ry, rx, q) == L.MA_EINVAL
        assert b"radii" in lib.ma_last_error()
    # more tiles than a launch holds: 2^23 blocks of 512 threads are 2^32 threads
    for H, W in ((1 << 24, 1 << 24), (1 << 16, 1 << 20), (1 << 20, 1 << 16), (1 << 13, 1 << 23)):
        assert f(ctx, p, L.MA_U8, H, W, L.MA_MORPH_ERODE, 1, 1, q) == L.MA_EINVAL
        assert b"too large" in lib.ma_last_error()


def test_header_library_and_bindings_agree():
    import re
    from microaligner_amd import _lib as L, build
    from _measured_path import HASH
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "microaligner_morphology.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", code))) == ["ma_morphology"] == sorted(L.MORPH_SIGNATURES)
    vals = {k: int(v) for k, v in re.findall(r"\b(MA_MORPH_[A-Z_]+)\s*=\s*(\d+)", code)}
    vals.update({k: int(v) for k, v in re.findall(r"#define\s+(MA_MORPH_[A-Z_]+)\s+(\d+)", code)})
    assert len(vals) == 7
    for name, v in vals.items():
        assert getattr(L, name) == v, name
    res, args = L.MORPH_SIGNATURES["ma_morphology"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    assert hasattr(L.load(), "ma_morphology")
    # off the measured path: the hash is the one the tests of the measured path hold, and the library's
    assert "morphology.hip" in build.SOURCES and build.source_hash() == HASH == L.source_hash()
    assert [os.path.basename(h) for h in build.SOURCE_HEADERS["morphology.hip"]] == ["microaligner_morphology.h"]
    src = open(os.path.join(build.CSRC, "morphology.hip")).read()
    assert "MA_REQUIRE_ALIGNED" not in src


def test_the_registry_holds_the_entry():
    """with the cases' module imported (here and by tests/test_gpu_morphology.py, before the two suites that run the registry
    are collected) the completeness check of tests/test_debug_fill.py holds for the new entry"""
    assert "ma_morphology" in G.declared_entries() and "ma_morphology" not in G.EXEMPT
    assert sum("ma_morphology" in c.entries for c in G.CASES) == 3
    from microaligner_amd import _lib as L
    tables = {n: d for n, d in vars(L).items() if n.endswith("SIGNATURES") and isinstance(d, dict)}
    entries = {name for d in tables.values() for name in d}
    assert G.declared_entries() | set(G.EXEMPT) == entries
