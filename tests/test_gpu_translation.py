"""-m gpu: the translation search on the device against the numpy statement of include/microaligner_translation.h
(tests/_translation_ref.py) -- the five u64 tables equal entry for entry, the peak rule on a case with tied scores, and
align_translation bit for bit against the statement's level loop over the oracle."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _translation_ref as R  # noqa: E402
import test_translation_ref as T  # noqa: E402
from microaligner_amd import TranslationInfo, align_translation, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
U8, U16, F32 = np.uint8, np.uint16, np.float32


def random_pair(shape, seed=5):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape, dtype=U8), rng.integers(0, 256, shape, dtype=U8)


def constant_moments(shape, window, value):
    """the statement for two images that are `value` everywhere: every sum is n(d) times a constant"""
    dx0, dx1, dy0, dy1 = window
    n = np.array([[R.count(shape[0], shape[1], dx, dy) for dx in range(dx0, dx1 + 1)] for dy in range(dy0, dy1 + 1)], np.uint64)
    v = np.uint64(value)
    return np.stack([n * v * v, n * v, n * v * v, n * v, n * v * v])


def check_tables(ctx, a, b, window, exp=None):
    got = ctx.translation_moments(ctx.asdevice(a), ctx.asdevice(b), window)
    exp = R.moments(a, b, window) if exp is None else exp
    assert got.dtype == np.uint64 and got.shape == exp.shape == (5, window[3] - window[2] + 1, window[1] - window[0] + 1)
    for k, name in enumerate(("S_ab", "S_a", "S_aa", "S_b", "S_bb")):
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, (name, len(bad), [(int(j) + window[2], int(i) + window[0], int(got[k, j, i]), int(exp[k, j, i]))
                                                for j, i in bad[:5]])
    return got


# 37 x 515: five strips of 128 columns, the last ragged, one ragged tile row, 17 x 2 blocks of shifts, shifts without an
# overlap on both sides of x; 96 x 161: three tile rows, an odd width, 6 x 4 blocks of shifts; 257 x 190: an off-centre window of
# 7 x 7 shifts (two quads a row, 16 threads a quad), a width that is no multiple of 4; 20 x 33: most shifts have n = 0
@pytest.mark.parametrize("shape,window", [((37, 515), (-257, 257, -18, 18)), ((96, 161), (-80, 80, -48, 48)),
                                          ((257, 190), (-40, -34, 52, 58)), ((20, 33), (-40, 40, -25, 25))])
def test_tables_equal_the_statement(ctx, shape, window):
    a, b = random_pair(shape)
    got = check_tables(ctx, a, b, window)
    if shape == (20, 33):
        assert (got[:, :, :8] == 0).all() and (got[:, :6] == 0).all() and (got[:, :, -8:] == 0).all()      # |dx| >= 33, |dy| >= 20


@pytest.mark.parametrize("window", [(0, 0, 0, 0), (5, 5, -7, -7), (-160, -160, 95, 95), (161, 161, 0, 0), (-3, 2, 40, 40),
                                    (17, 17, -50, 60)])
def test_a_single_shift_a_row_and_a_column_of_shifts(ctx, window):
    a, b = random_pair((96, 161), 6)
    check_tables(ctx, a, b, window)


@pytest.mark.parametrize("shape,window", [((1, 64), (-70, 70, -2, 2)), ((64, 1), (-2, 2, -70, 70)), ((1, 1), (-1, 1, -1, 1)),
                                          ((2, 3), (-3, 3, -2, 2))])
def test_degenerate_images(ctx, shape, window):
    a, b = random_pair(shape, 7)
    check_tables(ctx, a, b, window)


def test_every_partial_sum_at_its_maximum(ctx):
    """130 x 128 of 255 over every shift with an overlap and one more each way: whole tiles of 255 * 255 products, the u32
    partial sums as large as the decomposition lets them get"""
    shape, window = (130, 128), (-128, 128, -130, 130)
    a = np.full(shape, 255, U8)
    check_tables(ctx, a, a, window, constant_moments(shape, window, 255))
    small, win = (40, 36), (-36, 36, -40, 40)                 # the closed form itself against the slices
    assert np.array_equal(constant_moments(small, win, 255), R.moments(np.full(small, 255, U8), np.full(small, 255, U8), win))


def test_sums_beyond_32_bits(ctx):
    """600 x 700 of 255, 25 shifts about (301, -212): S_ab = n * 65025 is 7.5e9 and more, above 2^32"""
    shape, window = (600, 700), (299, 303, -214, -210)
    a = np.full(shape, 255, U8)
    got = check_tables(ctx, a, a, window, constant_moments(shape, window, 255))
    assert int(got[0].min()) > 1 << 32
    check_tables(ctx, *random_pair(shape, 8), window)


def test_all_zero_images_have_no_score(ctx):
    z = np.zeros((50, 70), U8)
    got = check_tables(ctx, z, z, (-9, 9, -6, 6))
    assert not got.any()
    res = ctx.translation_search(ctx.asdevice(z), ctx.asdevice(z), (-9, 9, -6, 6), exclude=2, table=True)
    assert np.isnan(res["table"]).all() and not res["valid"] and not res["at_limit"]
    assert (res["dx"], res["dy"], res["n"], res["delta_x"], res["delta_y"]) == (0, 0, 0, 0.0, 0.0)
    assert np.isnan(res["score"]) and np.isnan(res["second"])
    a, _ = random_pair((50, 70), 9)
    for x, y in ((a, z), (z, a)):                                # one side without variance
        assert not ctx.translation_search(ctx.asdevice(x), ctx.asdevice(y), (-2, 2, -2, 2))["valid"]


def same(got, exp):
    """every field of a search result, bit for bit (NaN equal to NaN)"""
    for k in ("dx", "dy", "n", "at_limit", "valid"):
        assert got[k] == exp[k], (k, got[k], exp[k])
    for k in ("delta_x", "delta_y", "score", "second"):
        assert got[k] == exp[k] or (math.isnan(got[k]) and math.isnan(exp[k])), (k, got[k], exp[k])


def test_search_follows_the_peak_rule_on_tied_scores(ctx):
    """a = b, periodic by 8 along x and 6 along y and mirror-symmetric along x: the moments at (dx, dy) and (-dx, dy) are the
    same integers, so those scores are equal to the bit, and the window leaves out d = 0"""
    rng = np.random.default_rng(10)
    half = rng.integers(0, 256, (6, 4), dtype=U8)
    a = np.tile(np.concatenate([half, half[:, ::-1]], axis=1), (8, 8))
    assert a.shape == (48, 64) and np.array_equal(a, a[:, ::-1]) and np.array_equal(a[:, 8:], a[:, :-8])
    window = (-9, 9, 5, 7)
    d_a = ctx.asdevice(a)
    for exclude in (0, 2, 30):
        exp, table = R.search(a, a, window, exclude)
        assert table[1, 1] == table[1, 17] > 0.999 and np.array_equal(table, table[:, ::-1])
        got = ctx.translation_search(d_a, d_a, window, exclude=exclude, table=True)
        assert np.array_equal(got["table"], table, equal_nan=True)
        same(got, exp)
        plain = ctx.translation_search(d_a, d_a, window, exclude=exclude)
        assert plain["table"] is None
        same(plain, exp)
    assert np.isnan(exp["second"]) and exp["dy"] == 6
    b = np.roll(a, (1, 3), axis=(0, 1))                          # an off-centre window with the peak inside: a refinement
    exp, table = R.search(a, b, (-2, 9, -4, 3), 1)
    got = ctx.translation_search(d_a, ctx.asdevice(b), (-2, 9, -4, 3), exclude=1, table=True)
    assert np.array_equal(got["table"], table, equal_nan=True)
    same(got, exp)


# ---- align_translation ------------------------------------------------------------------------------------------------------
_expected = {}


def pair(name):
    if name == "cells-dog":
        return T.integer_pair("cells", *T.INTEGER_CASES[0][:2]) + ("dog", T.INTEGER_CASES[0][2])
    if name == "field-u8":
        return T.integer_pair("field", *T.INTEGER_CASES[1][:2]) + ("u8", T.INTEGER_CASES[1][2])
    if name == "cells-u8":
        return T.integer_pair("cells", *T.INTEGER_CASES[2][:2]) + ("u8", T.INTEGER_CASES[2][2])
    if name == "subpixel":
        return T.subpixel_pair(*T.SUBPIXEL_CASES[2][:2], 2.5) + ("u8", T.SUBPIXEL_CASES[2][2])
    return synthetic.make_unrelated_pair(200, 232, 4, U16) + ("u8", 100)


def expected(name):
    """the statement's loop over the oracle, once per pair"""
    if name not in _expected:
        ref, mov, labels, coarse = pair(name)
        _expected[name] = T.run_ref(ref, mov, labels, coarse)
    return _expected[name]


def check_against_the_loop(got, info, exp, exp_info):
    assert isinstance(info, TranslationInfo) and got.dtype == np.float64 and got.shape == (2, 3)
    assert np.array_equal(got, exp)
    assert info.shift == exp_info["shift"] and info.valid == exp_info["valid"] and info.accepted == exp_info["accepted"]
    assert info.at_limit == exp_info["at_limit"]
    for k in ("score", "score0", "distinct"):
        g, e = getattr(info, k), exp_info[k]
        assert g == e or (math.isnan(g) and math.isnan(e)), (k, g, e)
    assert len(info.levels) == len(exp_info["levels"])
    for lv, e in zip(info.levels, exp_info["levels"]):
        assert (lv.level, lv.shape, lv.window, lv.peak, lv.n, lv.at_limit) == \
            (e["level"], e["shape"], e["window"], e["peak"], e["n"], e["at_limit"]), (lv, e)
        assert lv.score == e["score"] and (lv.second == e["second"] or (math.isnan(lv.second) and math.isnan(e["second"]))), (lv, e)


@pytest.mark.parametrize("name", ["cells-dog", "field-u8", "cells-u8", "subpixel"])
def test_align_translation_is_the_statements_loop_bit_for_bit(ctx, name):
    ref, mov, labels, coarse = pair(name)
    exp, exp_info = expected(name)
    got, info = align_translation(ref, mov, labels=labels, coarse_side=coarse, return_info=True)
    check_against_the_loop(got, info, exp, exp_info)
    assert info.accepted and info.levels[-1].level == 0
    assert np.array_equal(align_translation(ref, mov, labels=labels, coarse_side=coarse), exp)


def test_align_translation_from_device_arrays(ctx):
    ref, mov, labels, coarse = pair("cells-u8")
    exp, exp_info = expected("cells-u8")
    got, info = align_translation(ctx.asdevice(ref), ctx.asdevice(mov), labels=labels, coarse_side=coarse, return_info=True)
    check_against_the_loop(got, info, exp, exp_info)
    got, info = align_translation(ctx.asdevice(ref), mov, labels=labels, coarse_side=coarse, return_info=True)
    check_against_the_loop(got, info, exp, exp_info)


def test_the_matrix_lands_mov_on_ref(ctx):
    from microaligner_amd import transform_img_with_tmat
    ref, mov, labels, coarse = pair("cells-u8")
    shape, shift = T.INTEGER_CASES[2][:2]
    tmat, info = align_translation(ref, mov, labels=labels, coarse_side=coarse, return_info=True)
    out = transform_img_with_tmat(mov, shape, tmat)
    y0, y1, x0, x1 = R.overlap(shape[0], shape[1], *shift)
    # the matrix carries the parabola's part (ex, ey), thousandths of a pixel: a bilinear sample that far from a pixel differs
    # from it by at most (ex + ey) times the image's range, and the cast back to uint16 rounds
    ex, ey = abs(info.shift[0] - shift[0]), abs(info.shift[1] - shift[1])
    assert ex <= 0.5 and ey <= 0.5
    bound = (ex + ey + 1e-9) * (float(mov.max()) - float(mov.min())) + 1.0
    assert out.dtype == ref.dtype and np.abs(out[y0:y1, x0:x1].astype(np.float64) - ref[y0:y1, x0:x1]).max() <= bound


def test_an_unrelated_pair_comes_back_with_the_statements_verdict(ctx):
    ref, mov, labels, coarse = pair("unrelated")
    exp, exp_info = expected("unrelated")
    got, info = align_translation(ref, mov, labels=labels, coarse_side=coarse, return_info=True)
    check_against_the_loop(got, info, exp, exp_info)
    strict, strict_info = align_translation(ref, mov, labels=labels, coarse_side=coarse, min_score=0.5, return_info=True)
    assert not strict_info.accepted and np.array_equal(strict, np.eye(2, 3)) and strict_info.shift == info.shift
    assert info.score < 0.5


def test_limits_reach_the_device_as_the_statement_has_them(ctx):
    ref, mov, labels, coarse = pair("cells-u8")
    O = T.oracle()
    for kw in (dict(finest_level=1), dict(max_shift=3), dict(refine_radius=1, exclude=0), dict(min_overlap=0.9),
               dict(finest_level=5)):
        exp, exp_info = R.align_translation_ref(ref, mov, O.pyr_down, T.make_labels(labels, O), coarse_side=coarse, **kw)
        got, info = align_translation(ref, mov, labels=labels, coarse_side=coarse, return_info=True, **kw)
        check_against_the_loop(got, info, exp, exp_info)
