"""Global translation search on the CPU (no GPU): the numpy statement of include/microaligner_translation.h
(tests/_translation_ref.py) with the oracle's pyr_down / normalize_minmax_u8 / dog -- whole-pixel crops of one canvas
recovered exactly, sub-pixel shifts within the parabola's bound, the sign of the matrix through the oracle's affine warp --
the host entry ma_translation_scores against Python integers where 64-bit arithmetic wraps, argument validation before any
device work, the CLI key, and the header against the built library and _lib.TRANSLATION_SIGNATURES."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _translation_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_translation.h")
F32, U8, U16 = np.float32, np.uint8, np.uint16
# build.source_hash() covers exactly these sources, then build.HEADERS, then the compiler flags: what it covered before this
# feature (tests/test_residual_shift_ref.py keeps the same list)
MEASURED_PATH_SOURCES = ["ma_api.hip", "farneback.hip", "remap.hip", "pyramid.hip", "dog.hip", "nmi.hip", "register.hip"]

# (shape, shift (dx, dy), coarse_side): ref(p) = mov(p + shift)
INTEGER_CASES = [((400, 520), (63, -97), 160), ((300, 333), (-140, 120), 100), ((257, 190), (5, 3), 64)]
SUBPIXEL_CASES = [((300, 333), (-41.3, 27.6), 100), ((200, 232), (17.75, -60.4), 100), ((257, 190), (3.5, 2.5), 64),
                  ((130, 515), (100.2, -9.9), 160)]
SUBPIXEL_BOUND = 0.05      # px: the project's bound for this parabola rule (tests/test_residual_shift_ref.py)


def oracle():
    from oracle import oracle as O
    O.build()
    return O


def make_labels(kind, O=None):
    O = O or oracle()
    if kind == "u8":
        return lambda img: img if img.dtype == U8 else O.normalize_minmax_u8(img)

    def dog(img):
        return np.zeros(img.shape, U8) if img.max() == 0 else O.dog(img, flags=0)
    return dog


_canvas = {}


def canvas(kind, shape):
    """one image of `shape` per generator, made once: 'cells' -- synthetic.make_cells uint16, 'field' -- the reference of
    synthetic.make_pair float32"""
    from microaligner_amd import synthetic
    if (kind, shape) not in _canvas:
        H, W = shape
        _canvas[kind, shape] = synthetic.make_cells(H, W, seed=3, dtype=U16) if kind == "cells" else \
            synthetic.make_pair(H, W, 3, F32, shift=(0.0, 0.0), amp=0.0)[0]
    return _canvas[kind, shape]


def integer_pair(kind, shape, shift):
    """(ref, mov), two crops of one canvas with ref(p) = mov(p + shift) wherever both hold p"""
    (h, w), (dx, dy) = shape, shift
    m = 160
    big = canvas(kind, (h + 2 * m, w + 2 * m))
    ref = np.ascontiguousarray(big[m:m + h, m:m + w])
    mov = np.ascontiguousarray(big[m - dy:m - dy + h, m - dx:m - dx + w])
    return ref, mov


def subpixel_pair(shape, shift, sigma, seed=11):
    """u8 crops of a Gaussian texture and of its cubic-spline interpolant moved by `shift`: ref(p) ~ mov(p + shift)"""
    from scipy.ndimage import gaussian_filter, shift as spline_shift
    (h, w), (dx, dy) = shape, shift
    m = 160
    tex = gaussian_filter(np.random.default_rng(seed).standard_normal((h + 2 * m, w + 2 * m)), sigma, mode="wrap")
    tex = (tex - tex.min()) * (255.0 / (tex.max() - tex.min()))
    moved = spline_shift(tex, (dy, dx), order=3, mode="grid-wrap")            # moved(p + d) = tex(p)
    crop = lambda img: np.ascontiguousarray(np.clip(np.rint(img[m:m + h, m:m + w]), 0, 255).astype(U8))   # noqa: E731
    return crop(tex), crop(moved)


def run_ref(ref, mov, labels, coarse_side, **kw):
    O = oracle()
    return R.align_translation_ref(ref, mov, O.pyr_down, make_labels(labels, O), coarse_side=coarse_side, **kw)


# ---- the statement against brute force ---------------------------------------------------------------------------------------
def test_statement_equals_brute_force_on_tiny_inputs():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (7, 9), dtype=U8)
    b = rng.integers(0, 256, (7, 9), dtype=U8)
    window = (-10, 10, -7, 8)
    mom = R.moments(a, b, window)
    table = R.scores(a.shape, window, mom)
    al, bl = a.tolist(), b.tolist()
    for dy in range(window[2], window[3] + 1):
        for dx in range(window[0], window[1] + 1):
            ps = [(y, x) for y in range(7) for x in range(9) if 0 <= y + dy < 7 and 0 <= x + dx < 9]
            n = len(ps)
            assert n == R.count(7, 9, dx, dy)
            sums = [sum(al[y][x] * bl[y + dy][x + dx] for y, x in ps), sum(al[y][x] for y, x in ps),
                    sum(al[y][x] ** 2 for y, x in ps), sum(bl[y + dy][x + dx] for y, x in ps),
                    sum(bl[y + dy][x + dx] ** 2 for y, x in ps)]
            assert [int(v) for v in mom[:, dy - window[2], dx - window[0]]] == sums, (dx, dy)
            num, va, vb = n * sums[0] - sums[1] * sums[3], n * sums[2] - sums[1] ** 2, n * sums[4] - sums[3] ** 2
            got = table[dy - window[2], dx - window[0]]
            if n == 0 or va == 0 or vb == 0:
                assert np.isnan(got), (dx, dy)
            else:
                assert got == float(num) / (math.sqrt(float(va)) * math.sqrt(float(vb))), (dx, dy)
    assert np.isnan(table[:, 0]).all() and np.isnan(table[0]).all()            # |dx| = 10 >= w, dy = -7: n = 0
    assert np.isnan(table[7 + 6, 10 + 8])                                       # a single pixel: va = 0


def test_peak_rule():
    t = np.full((5, 7), 0.25)
    shape, window = (40, 40), (-3, 3, -2, 2)
    res = R.peak(shape, window, t, 1)
    assert (res["dx"], res["dy"], res["score"], res["second"], res["at_limit"], res["valid"]) == (0, 0, 0.25, 0.25, False, True)
    assert res["n"] == 1600 and res["delta_x"] == 0.0 and res["delta_y"] == 0.0          # den = 0: no refinement
    t[2, 3] = np.nan
    assert (lambda r: (r["dx"], r["dy"]))(R.peak(shape, window, t, 1)) == (0, -1)          # distance 1: the smallest dy
    t[1, 3] = np.nan
    assert (lambda r: (r["dx"], r["dy"]))(R.peak(shape, window, t, 1)) == (-1, 0)          # then the smallest dx
    # an off-centre window: the distance is that of the shift itself, not of the position in the table
    res = R.peak(shape, (5, 11, 3, 7), np.full((5, 7), 0.5), 0)
    assert (res["dx"], res["dy"], res["at_limit"], res["n"]) == (5, 3, True, 35 * 37)
    t[:] = np.nan
    res = R.peak(shape, window, t, 1)
    assert not res["valid"] and np.isnan(res["score"]) and np.isnan(res["second"]) and (res["dx"], res["dy"], res["n"]) == (0, 0, 0)
    t[2, 2:5] = (0.5, 0.9, 0.7)
    t[0, 0] = 0.8
    res = R.peak(shape, window, t, 1)
    assert res["delta_x"] == 0.5 * (0.5 - 0.7) / (0.5 - 2.0 * 0.9 + 0.7) and res["delta_y"] == 0.0      # beside a NaN along y
    assert res["second"] == 0.8 and not res["at_limit"]
    assert np.isnan(R.peak(shape, window, t, 3)["second"])                      # nothing lies more than 3 px away


# ---- whole-pixel shifts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,labels,case", [("cells", "u8", 0), ("cells", "dog", 0), ("field", "u8", 0), ("field", "dog", 0),
                                              ("cells", "u8", 1), ("field", "u8", 1), ("cells", "u8", 2), ("field", "u8", 2)])
def test_integer_crops_of_one_canvas_are_recovered_exactly(kind, labels, case):
    shape, shift, coarse = INTEGER_CASES[case]
    ref, mov = integer_pair(kind, shape, shift)
    tmat, info = run_ref(ref, mov, labels, coarse)
    print(kind, labels, shape, shift, [(lv["level"], lv["peak"], round(lv["score"], 4)) for lv in info["levels"]], info["shift"])
    assert info["valid"] and info["accepted"] and info["levels"][-1]["level"] == 0
    assert info["levels"][-1]["peak"] == shift
    # the parabola's part: at most half a pixel by construction (the labels of two crops differ near their borders, so the
    # neighbours of the peak are not symmetric and the part is not zero)
    assert abs(info["shift"][0] - shift[0]) <= 0.5 and abs(info["shift"][1] - shift[1]) <= 0.5
    assert info["score"] >= 0.98
    assert np.array_equal(tmat, [[1.0, 0.0, -info["shift"][0]], [0.0, 1.0, -info["shift"][1]]])


@pytest.mark.parametrize("dtype", [U8, U16])
def test_sign_the_matrix_lands_mov_on_ref(dtype):
    """the matrix of the whole-pixel shift, through the oracle's affine warp, gives ref on O(shift), bit for bit"""
    O = oracle()
    shape, shift, coarse = INTEGER_CASES[0]
    ref, mov = integer_pair("cells", shape, shift)
    if dtype == U8:
        lab = O.normalize_minmax_u8(canvas("cells", (shape[0] + 320, shape[1] + 320)))      # one scaling for both crops
        ref = np.ascontiguousarray(lab[160:160 + shape[0], 160:160 + shape[1]])
        mov = np.ascontiguousarray(lab[160 - shift[1]:160 - shift[1] + shape[0], 160 - shift[0]:160 - shift[0] + shape[1]])
    _, info = run_ref(ref, mov, "u8", coarse)
    assert info["levels"][-1]["peak"] == shift
    tmat = np.array([[1.0, 0.0, -shift[0]], [0.0, 1.0, -shift[1]]])
    out = O.warp_affine(mov, tmat)
    y0, y1, x0, x1 = R.overlap(shape[0], shape[1], *shift)
    assert out.dtype == dtype and np.array_equal(out[y0:y1, x0:x1], ref[y0:y1, x0:x1])
    assert not np.array_equal(O.warp_affine(mov, np.array([[1.0, 0.0, shift[0]], [0.0, 1.0, shift[1]]]))[y0:y1, x0:x1],
                              ref[y0:y1, x0:x1])


# ---- sub-pixel shifts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SUBPIXEL_CASES)))
def test_subpixel_shifts_within_the_parabola_bound(case):
    """Gaussian textures of sigma 1.5, 2.5 and 4 px moved by a cubic spline; the bound is the project's 0.05 px for this
    parabola rule.  Measured with this statement: 0.0023 - 0.037 px."""
    shape, shift, coarse = SUBPIXEL_CASES[case]
    for sigma in (1.5, 2.5, 4.0):
        ref, mov = subpixel_pair(shape, shift, sigma)
        _, info = run_ref(ref, mov, "u8", coarse)
        err = math.hypot(info["shift"][0] - shift[0], info["shift"][1] - shift[1])
        print(f"{shape} shift {shift} sigma {sigma}: found {info['shift']}, off by {err:.4f} px, score {info['score']:.4f}")
        assert info["valid"] and info["accepted"] and err <= SUBPIXEL_BOUND, (sigma, info["shift"], err)


def test_finest_level_and_max_shift_limit_the_search():
    shape, shift, coarse = INTEGER_CASES[0]
    ref, mov = integer_pair("field", shape, shift)
    _, info = run_ref(ref, mov, "u8", coarse, finest_level=1)
    assert [lv["level"] for lv in info["levels"]] == [2, 1]
    assert abs(info["shift"][0] - shift[0]) <= 1.0 and abs(info["shift"][1] - shift[1]) <= 1.0
    _, info = run_ref(ref, mov, "u8", coarse, max_shift=40)                    # the truth is out of reach
    assert info["levels"][0]["window"] == (-10, 10, -10, 10) and info["levels"][-1]["window"][0] >= -40
    assert info["levels"][-1]["peak"] != shift
    ref, mov = integer_pair("field", (64, 80), (7, -5))
    _, info = run_ref(ref, mov, "u8", 1 << 20)                                  # a single level: level 0 itself, exhaustive
    assert [lv["level"] for lv in info["levels"]] == [0] and info["levels"][0]["peak"] == (7, -5)
    assert info["levels"][0]["window"] == (-40, 40, -32, 32)


# ---- ma_translation_scores ------------------------------------------------------------------------------------------------
def _lib_scores(h, w, window, mom):
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    dx0, dx1, dy0, dy1 = window
    mom = np.ascontiguousarray(mom, np.uint64)
    out = np.empty(mom.shape[1:])
    rc = lib.ma_translation_scores(h, w, dx0, dx1, dy0, dy1, mom.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                   out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == _lib.MA_OK, lib.ma_last_error()
    return out


def _two_level_moments(n, p, q, r, lo_a=0, lo_b=0):
    """moments of images nobody builds: a is 255 on p of n pixels and lo_a elsewhere, b is 255 on q and lo_b elsewhere, both
    255 on r"""
    S_a, S_aa = 255 * p + lo_a * (n - p), 255 * 255 * p + lo_a * lo_a * (n - p)
    S_b, S_bb = 255 * q + lo_b * (n - q), 255 * 255 * q + lo_b * lo_b * (n - q)
    S_ab = 255 * 255 * r + 255 * lo_b * (p - r) + lo_a * 255 * (q - r) + lo_a * lo_b * (n - p - q + r)
    return [S_ab, S_a, S_aa, S_b, S_bb]


def test_scores_entry_follows_python_integers_beyond_64_bits():
    """a 16384 x 16384 image (2^28 pixels), the moments made arithmetically: n * S_ab passes 2^71 and num itself passes 2^63,
    so 64-bit arithmetic, wrapping or not, gives other scores"""
    h = w = 16384
    window = (-2, 2, -1, 1)
    mom = np.zeros((5, 3, 5), np.uint64)
    wrapped, widest, va_widest = 0, 0, 0
    for j in range(3):
        for i in range(5):
            n = R.count(h, w, window[0] + i, window[2] + j)
            k = 5 * j + i
            if k % 3 == 0:        # about half bright, correlated: num ~ 2^68
                m = _two_level_moments(n, n // 2 + k, n // 2 - 7 * k, n // 3 + k, lo_a=1, lo_b=2)
            elif k % 3 == 1:      # every sum near its maximum
                m = _two_level_moments(n, n - 3 - k, n - 5, n - 8 - k, lo_a=254, lo_b=3)
            else:                 # anti-correlated: num < -2^63
                m = _two_level_moments(n, n // 2, n // 2 + k, k)
            mom[:, j, i] = m
            num = n * m[0] - m[1] * m[3]
            wrapped += abs(num) >= 1 << 63
            widest, va_widest = max(widest, n * m[0]), max(va_widest, n * m[2] - m[1] ** 2)
    assert wrapped >= 8 and widest >= 1 << 71 and va_widest >= 1 << 64
    got = _lib_scores(h, w, window, mom)
    exp = R.scores((h, w), window, mom)
    assert np.isfinite(exp).all() and (np.abs(exp) <= 1.0 + 1e-12).all()
    assert np.array_equal(got, exp), (got, exp)


def test_scores_entry_gives_nan_without_pixels_or_variance():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (6, 5), dtype=U8)
    b = rng.integers(0, 256, (6, 5), dtype=U8)
    window = (-6, 6, -7, 7)
    mom = R.moments(a, b, window)
    got, exp = _lib_scores(6, 5, window, mom), R.scores((6, 5), window, mom)
    assert np.array_equal(got, exp, equal_nan=True)
    assert np.isnan(got[:, :2]).all() and np.isnan(got[:2]).all() and np.isfinite(got[7, 6])      # n = 0 at |dx| >= 5, |dy| >= 6
    mom[:] = 12345                                                              # n = 0 whatever the table holds
    assert np.isnan(_lib_scores(6, 5, (5, 9, -1, 1), mom[:, :3, :5])).all()
    flat = np.full((6, 5), 9, U8)
    for x, y in ((flat, b), (a, flat), (flat, flat)):                           # va = 0, vb = 0, both
        m = R.moments(x, y, (-1, 1, -1, 1))
        assert np.isnan(_lib_scores(6, 5, (-1, 1, -1, 1), m)).all() and np.isnan(R.scores((6, 5), (-1, 1, -1, 1), m)).all()
    b2 = b.copy()
    b2[:, 1:] = 200                                                             # vb = 0 only where column 0 of b is left out
    m = R.moments(a, b2, (0, 1, 0, 0))
    s = _lib_scores(6, 5, (0, 1, 0, 0), m)
    assert np.isfinite(s[0, 0]) and np.isnan(s[0, 1])


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_arguments_are_validated_before_the_device(monkeypatch):
    import microaligner_amd.device as dev
    from microaligner_amd import align_translation
    from microaligner_amd.feature_reg import translation as T
    monkeypatch.setattr(T, "get_context", lambda *a: pytest.fail("a device was asked for"))
    monkeypatch.setattr(dev, "get_context", lambda *a: pytest.fail("a device was asked for"))
    a = np.zeros((64, 80), F32)
    for kw in (dict(mov_img=np.zeros((64, 81), F32)), dict(mov_img=np.zeros((64, 80), np.int32)), dict(ref_img=np.zeros((2, 64, 80), F32)),
               dict(labels="raw"), dict(labels=None), dict(min_overlap=0.0), dict(min_overlap=1.5), dict(min_overlap=-0.1),
               dict(min_overlap="half"), dict(refine_radius=0), dict(refine_radius=1.5), dict(coarse_side=31), dict(coarse_side=0),
               dict(finest_level=-1), dict(exclude=-1), dict(max_shift=-1), dict(min_score=float("nan"))):
        with pytest.raises(ValueError):
            align_translation(**dict(dict(ref_img=a, mov_img=a), **kw))
    big = np.lib.stride_tricks.as_strided(np.zeros(1, U8), (4000, 4000), (0, 0))          # no memory behind it
    with pytest.raises(ValueError, match="coarse_side"):                        # 4001 x 4001 shifts at the only level
        align_translation(big, big, coarse_side=4000)
    # the same size passes the checks once the coarsest window fits
    assert T.check_arguments(big, big, "dog", None, 0.5, 512, 2, 0, 2, None) == [(4000, 4000), (2000, 2000), (1000, 1000), (500, 500)]
    assert T.check_arguments(big, big, "dog", 100, 0.5, 4000, 2, 0, 2, None) == [(4000, 4000)]
    assert T.level_shapes((257, 190), 64) == [(257, 190), (129, 95), (65, 48)]  # 33 x 24 would be below 32
    assert T.level_limits((65, 48), 2, None, 0.5) == (24, 32) and T.level_limits((65, 48), 2, 50, 0.5) == (13, 13)
    assert T.level_window((24, 32), None, 2) == (-24, 24, -32, 32)
    assert T.level_window((48, 64), (24, -32), 2) == (46, 48, -64, -62)
    assert T.level_window((47, 64), (24, 3), 1) == (46, 47, 5, 7)                # the centre is brought within the limits first
    ok = np.zeros((10, 12), U8)
    for kw in (dict(ref=np.zeros((10, 12), F32)), dict(mov=np.zeros((10, 13), U8)), dict(window=(0, 1, 2)), dict(window=(1, 0, 0, 0)),
               dict(window=(0, 0, 1, 0)), dict(window=(0.0, 1, 0, 1)), dict(window=(-512, 512, -512, 512)), dict(window=None),
               dict(exclude=-1), dict(exclude=1.5), dict(window=(0, 1 << 31, 0, 0))):
        with pytest.raises(ValueError):
            dev.translation_params(**dict(dict(ref=ok, mov=ok, window=(-1, 1, -1, 1)), **kw))
    assert dev.translation_params(ok, ok, (-40, 40, 3, 3), 2) == (10, 12, -40, 40, 3, 3, 2)
    assert dev.translation_params(ok, ok, (-511, 512, -512, 511)) == (10, 12, -511, 512, -512, 511, 0)    # 2^20 exactly


def test_c_entries_return_einval_without_a_device():
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    p = C.c_void_p(0x1000)            # never dereferenced: every call below fails its checks
    mom = (C.c_ulonglong * 64)()
    sc = (C.c_double * 64)()
    res = _lib.TranslationResult()
    good = dict(h=40, w=30, dx0=-1, dx1=1, dy0=-1, dy1=1)
    bad = [dict(h=0), dict(w=0), dict(h=-3), dict(h=65537, w=65537), dict(h=1 << 30, w=8), dict(dx1=-2), dict(dy0=2),
           dict(dx0=-512, dx1=512, dy0=-512, dy1=512), dict(dx0=-(1 << 31), dx1=(1 << 31) - 1), dict(dy0=0, dy1=1 << 20)]

    def moments(ctx=p, ref=p, mov=p, out=mom, **kw):
        g = dict(good, **kw)
        return lib.ma_translation_moments(ctx, ref, mov, g["h"], g["w"], g["dx0"], g["dx1"], g["dy0"], g["dy1"], out)

    def search(ctx=p, ref=p, mov=p, exclude=2, out=C.byref(res), **kw):
        g = dict(good, **kw)
        return lib.ma_translation_search(ctx, ref, mov, g["h"], g["w"], g["dx0"], g["dx1"], g["dy0"], g["dy1"], exclude, out, None)

    def scores(m=mom, out=sc, **kw):
        g = dict(good, **kw)
        return lib.ma_translation_scores(g["h"], g["w"], g["dx0"], g["dx1"], g["dy0"], g["dy1"], m, out)
    for kw in (dict(ctx=None), dict(ref=None), dict(mov=None), dict(out=None)):
        assert moments(**kw) == _lib.MA_EINVAL and search(**kw) == _lib.MA_EINVAL, kw
        assert b"NULL" in lib.ma_last_error()
    assert scores(m=None) == _lib.MA_EINVAL and scores(out=None) == _lib.MA_EINVAL
    for kw in bad:
        assert moments(**kw) == _lib.MA_EINVAL and search(**kw) == _lib.MA_EINVAL and scores(**kw) == _lib.MA_EINVAL, kw
    assert moments(dx0=-512, dx1=512, dy0=-512, dy1=512) == _lib.MA_EINVAL and b"2^20" in lib.ma_last_error()
    assert moments(h=65537, w=65537) == _lib.MA_EINVAL and b"2^32" in lib.ma_last_error()
    assert search(exclude=-1) == _lib.MA_EINVAL and b"exclude" in lib.ma_last_error()
    assert scores() == _lib.MA_OK                                               # the host entry needs no ctx and no device


# ---- the CLI key, the header, the build recipe ----------------------------------------------------------------------------
def test_translation_fallback_schema():
    from microaligner_amd import pipeline
    base = dict(NumberPyramidLevels=3, NumberIterationsPerLevel=3, TileSize=1000, Overlap=100, NumberOfWorkers=0,
                UseFullResImage=False, UseDOG=True)
    assert pipeline.RegParam(dict(base)).TranslationFallback is False
    assert pipeline.RegParam(dict(base, TranslationFallback=True)).TranslationFallback is True
    assert pipeline.RegParam(dict(base, TranslationFallback=False)).TranslationFallback is False
    for bad in (1, None, "true", [True]):
        with pytest.raises(TypeError):
            pipeline.RegParam(dict(base, TranslationFallback=bad))
    with pytest.raises(ValueError, match="FeatureReg only"):
        pipeline.RegParam(dict(base, TranslationFallback=True), optflow=True)
    assert pipeline.RegParam(dict(base, DirectRefine="affine", TranslationFallback=True)).DirectRefine == "affine"


def test_translation_fallback_replaces_only_the_identity(monkeypatch):
    import microaligner_amd
    from microaligner_amd import pipeline
    from microaligner_amd.feature_reg.translation import TranslationInfo
    calls, lines = [], []
    found = np.array([[1.0, 0.0, -12.5], [0.0, 1.0, 7.0]])

    def fake(ref, mov, return_info=False, accepted=True):
        calls.append((ref, mov))
        info = TranslationInfo([], (12.5, -7.0), 0.9, 0.1, 0.4, False, True, fake.accepted)
        return (found if fake.accepted else np.eye(2, 3)), info
    fake.accepted = True
    monkeypatch.setattr(microaligner_amd, "align_translation", fake)
    img = np.zeros((4, 4), U8)
    other = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, 0.0]])
    assert pipeline.translation_fallback(img, img, other, lines.append) is other and not calls and not lines
    out = pipeline.translation_fallback(img, img, np.eye(2, 3), lines.append)
    assert np.array_equal(out, found) and len(calls) == 1
    assert "12.50" in lines[0] and "-7.00" in lines[0] and "0.9000" in lines[0] and "0.4000" in lines[0] and "True" in lines[0]
    fake.accepted = False
    eye = np.eye(2, 3)
    assert pipeline.translation_fallback(img, img, eye, lines.append) is eye and "False" in lines[1]


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ma_translation_[a-z0-9_]+)\s*\(", text))), text


def test_translation_header_library_and_bindings_agree():
    import microaligner_amd
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    names, text = _declared(HEADER)
    assert names == ["ma_translation_moments", "ma_translation_scores", "ma_translation_search"] == sorted(_lib.TRANSLATION_SIGNATURES)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_translation.h but not exported"
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, text, flags=re.S).group(1)
        restype, argtypes = _lib.TRANSLATION_SIGNATURES[n]
        assert restype is C.c_int and len(proto.split(",")) == len(argtypes), n
        for p, t in zip((s.strip() for s in proto.split(",")), argtypes):
            if p.startswith("int "):
                assert t is C.c_int, (n, p)
            elif "unsigned long long*" in p:
                assert t is C.POINTER(C.c_ulonglong), (n, p)
            elif p.startswith("double*"):
                assert t is C.POINTER(C.c_double), (n, p)
            elif "ma_translation_result*" in p:
                assert t is C.POINTER(_lib.TranslationResult), (n, p)
            else:
                assert t is C.c_void_p, (n, p)
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.DIRECT_SIGNATURES, _lib.LANDMARK_SIGNATURES]
    assert not any(set(_lib.TRANSLATION_SIGNATURES) & set(t) for t in others)
    # the struct, field by field
    body = re.search(r"typedef struct ma_translation_result \{(.*?)\}", text, flags=re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"\b(?:int|double|long long)\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == [f for f, _ in _lib.TranslationResult._fields_]
    assert re.search(r"#define\s+MA_TRANSLATION_MAX_SHIFTS\s+\(1 << 20\)", text) and _lib.MA_TRANSLATION_MAX_SHIFTS == 1 << 20
    assert _lib.MA_TRANSLATION_MAX_PIXELS == 1 << 32
    assert {"align_translation", "TranslationInfo"} <= set(microaligner_amd.__all__)
    assert callable(microaligner_amd.align_translation)


def test_translation_stays_out_of_the_measured_path_hash():
    """translation.hip and its header are built but not hashed: build.source_hash() is what the sources of the measured path,
    build.HEADERS and the flags give, as before the feature"""
    import hashlib
    from microaligner_amd import build
    assert "translation.hip" in build.SOURCES
    assert [os.path.abspath(h) for h in build.SOURCE_HEADERS["translation.hip"]] == [HEADER]
    assert HEADER not in [os.path.abspath(h) for h in build.HEADERS]
    hh = hashlib.sha256()
    for path in [os.path.join(build.CSRC, s) for s in MEASURED_PATH_SOURCES] + build.HEADERS:
        hh.update(open(path, "rb").read())
    hh.update(" ".join(build._flags()).encode())
    assert build.source_hash() == hh.hexdigest()[:16]
