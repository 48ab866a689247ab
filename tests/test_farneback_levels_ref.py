"""The CPU restatement of cv2.calcOpticalFlowFarneback with levels > 0 (tests/c_ref/farneback_levels_ref.c): pinned to the
single-scale oracle at levels = 0, its level table and resize checked against their formulas, the pyramid shown to find
the large motion a single scale misses, and the whole multi-level algorithm compared over the whole image with an
independent float64 statement (tests/_f64_ref.py), which is also shown to catch plausible convention errors.  The GPU
pyramid is compared with it in test_gpu_farneback_levels.py and with the float64 statement in
test_gpu_farneback_levels_f64.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _f64_ref import PYRAMID_ERRORS, farneback_float64, farneback_pyramid_float64, level_table  # noqa: E402
from _fb_levels_ref import LevelsRef  # noqa: E402

from microaligner_amd import synthetic  # noqa: E402
from oracle import oracle  # noqa: E402


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    r = LevelsRef(tmp_path_factory.mktemp("fb_levels_ref"))
    r.set_threads(min(8, os.cpu_count() or 1))
    return r


def _pair(H, W, dtype, seed=5, shift=(3.3, -2.1)):
    a, b = synthetic.make_pair(H, W, seed=seed, shift=shift)
    if dtype == np.uint8:
        return (np.clip(a, 0, 1) * 255).astype(np.uint8), (np.clip(b, 0, 1) * 255).astype(np.uint8)
    if dtype == np.uint16:
        return (np.clip(a, 0, 1) * 65535).astype(np.uint16), (np.clip(b, 0, 1) * 65535).astype(np.uint16)
    return a.astype(np.float32), b.astype(np.float32)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("win", [15, 51, 99])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_levels_zero_is_the_single_scale_oracle(ref, dtype, win, fused):
    mov, refimg = _pair(71, 93, dtype)
    for iters in (1, 2, 3):
        exp = oracle.calc_optical_flow_farneback(mov, refimg, win, iters, fused=fused)
        got = ref.farneback(mov, refimg, 0, win, iters, fused=fused)
        assert np.array_equal(got, exp, equal_nan=True), (iters, np.abs(got - exp).max())


def _cv_round(v):
    return int(round(v))  # Python rounds half to even, as cvRound does


@pytest.mark.parametrize("H,W,levels", [(1024, 768, 4), (1024, 768, 9), (101, 103, 2), (103, 101, 5), (300, 260, 9),
                                        (63, 200, 3), (64, 64, 1), (46000, 3000, 30)])
def test_level_table_follows_the_formulas(ref, H, W, levels):
    kept, scale = 0, 1.0
    for k in range(levels):
        scale *= 0.5
        if W * scale < 32 or H * scale < 32:
            break
        kept = k + 1
    table = ref.level_table(H, W, levels)
    assert len(table) == kept + 1
    for k, (w, h, ksize, sigma) in enumerate(table):
        s = 0.5 ** k
        assert sigma == (1 / s - 1) * 0.5
        assert ksize == max(_cv_round(sigma * 5) | 1, 3)
        assert (w, h) == (_cv_round(W * s), _cv_round(H * s))
    if len(table) > 4:
        assert [t[2] for t in table[1:5]] == [3, 9, 19, 39]


def test_level_sizes_round_half_to_even(ref):
    # 101 * 0.5 = 50.5 -> 50 and 103 * 0.5 = 51.5 -> 52
    assert ref.level_table(101, 103, 1)[1][:2] == (52, 50)
    assert ref.level_table(103, 101, 1)[1][:2] == (50, 52)


def _bilinear64(src, dw, dh):
    """float64 half-pixel bilinear resize with edge clamping; the source positions are rounded to float32 first, as
    cv::resize stores them"""
    sh, sw = src.shape[:2]
    x = np.clip(((np.arange(dw) + 0.5) * (sw / dw) - 0.5).astype(np.float32).astype(np.float64), 0, sw - 1)
    y = np.clip(((np.arange(dh) + 0.5) * (sh / dh) - 0.5).astype(np.float32).astype(np.float64), 0, sh - 1)
    x0 = np.minimum(np.floor(x).astype(int), sw - 1)
    y0 = np.minimum(np.floor(y).astype(int), sh - 1)
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    fx, fy = x - x0, y - y0
    s = src.astype(np.float64)
    if s.ndim == 3:
        fx, fy = fx[None, :, None], fy[:, None, None]
    else:
        fx, fy = fx[None, :], fy[:, None]
    top = s[y0][:, x0] * (1 - fx) + s[y0][:, x1] * fx
    bot = s[y1][:, x0] * (1 - fx) + s[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("shape,dsize,cn", [((101, 103), (52, 50), 1), ((517, 611), (153, 129), 1), ((517, 611), (76, 65), 1),
                                            ((65, 76), (153, 129), 2), ((50, 52), (103, 101), 2), ((37, 33), (33, 37), 1)])
def test_resize_matches_half_pixel_bilinear(ref, shape, dsize, cn, fused):
    rng = np.random.default_rng(7)
    src = (rng.random(shape + ((cn,) if cn > 1 else ())) + 0.5).astype(np.float32)
    got = ref.resize_linear(src, dsize, fused=fused)
    exp = _bilinear64(src, *dsize)
    assert got.shape == exp.shape
    np.testing.assert_allclose(got, exp, rtol=1e-6, atol=0)


def test_resize_by_exactly_two_is_the_2x2_mean(ref):
    rng = np.random.default_rng(8)
    src = rng.standard_normal((96, 130)).astype(np.float32)
    got = ref.resize_linear(src, (65, 48))
    exp = ((src[0::2, 0::2] + src[0::2, 1::2]) + (src[1::2, 0::2] + src[1::2, 1::2])) * np.float32(0.25)
    assert np.array_equal(got, exp)


def test_the_pyramid_finds_large_motion(ref):
    shift = (24, -17)
    refimg, mov = synthetic.make_pair(512, 512, seed=3, shift=shift)
    dx, dy = synthetic.displacement(512, 512, shift=shift)
    true = np.stack(np.broadcast_arrays(dx, dy), -1)
    err = {}
    for levels in (0, 4):
        flow = ref.farneback(mov, refimg, levels, 15, 3)
        e = np.hypot(*np.moveaxis(flow - true, -1, 0))[96:-96, 96:-96]
        err[levels] = float(np.median(e))
    assert err[4] < 0.5, err
    assert err[0] > 5, err


# ---- the whole pyramid against the independent float64 statement -------------------------------------------------------
def moving_pair(H, W, dtype, shift, amp=2.0, seed=5):
    """(prev, next) from make_pair: `prev` is the moved image, so the flow prev -> next varies in space (make_pair's
    sinusoidal field of amplitude `amp` around `shift`); a constant shift would hide flow-resize errors, as resizing a
    constant field gives the same constant under any convention.  dtype "mixed": uint8 prev, float32 next."""
    if dtype == "mixed":
        ref8, mov8 = synthetic.make_pair(H, W, seed=seed, dtype=np.uint8, shift=shift, amp=amp)
        _, mov = synthetic.make_pair(H, W, seed=seed, dtype=np.float32, shift=shift, amp=amp)
        return ref8, mov
    ref_, mov = synthetic.make_pair(H, W, seed=seed, dtype=dtype, shift=shift, amp=amp)
    return mov, ref_


def flow_gap(got, exp):
    """per-pixel max over (dx, dy) of |got - exp|, px"""
    return np.abs(np.asarray(got, np.float64) - exp).max(-1)


def assert_within(d, q99, dmax, what=""):
    assert np.quantile(d, 0.99) <= q99 and d.max() <= dmax, \
        f"{what}: 99th percentile {np.quantile(d, 0.99):.2e} px (bound {q99:.0e}), max {d.max():.2e} px (bound {dmax:.0e})"


# (H, W, levels, win, iterations, dtype, shift, amp, q99 bound, max bound).  The bounds hold over the WHOLE image in both
# rounding models; each is about 3x the larger gap measured in the two models (noted as q99 / max), which is float32
# storage in the restatement (expansions, matrices, window sums, resize coordinates) against float64 here.  Coverage:
# 1-4 levels, a level dropped by the 32-px clamp (103 x 101 and 256 x 320 at levels 2 and 4 keep 1 and 3), odd and even
# sides, level sizes that round half to even (101 -> 50, 103 -> 52, 130 / 4 -> 32, 520 / 16 -> 32), an even level 1 (the
# 2x area path: 256 x 320, 512 x 512), windows 15 - 301 (301 on the 32-row coarse level of 130 x 260), 1 and 3
# iterations, every input kind and a motion of tens of pixels.
PYRAMID_CASES = {
    # 1.6e-4 / 1.2e-3
    "256x320-L2-w15-i3-f32": (256, 320, 2, 15, 3, np.float32, (9.5, -6.25), 2.0, 7e-4, 4e-3),
    # 5.4e-5 / 2.7e-2: at one pixel (125, 307) of level 0, x + dx at the last UpdateMatrices lies 2.5e-6 px from the
    # right end of the sampling range (x1 = w - 2), so float32 and float64 fall on different sides of OpenCV's
    # out-of-range test there; the switch of that pixel's matrices spreads through the final window blur to a disc of
    # ~80 pixels, where the gap reaches 2.7e-2 px.  The rest of the image is as close as the other cases.
    "256x320-L3-w15-i3-f32": (256, 320, 3, 15, 3, np.float32, (9.5, -6.25), 2.0, 2e-4, 8e-2),
    # 3.8e-5 / 9.0e-5
    "101x103-L1-w15-i3-u8": (101, 103, 1, 15, 3, np.uint8, (3.3, -2.1), 2.0, 1.2e-4, 3e-4),
    # 2.6e-6 / 3.7e-6
    "103x101-L2-w99-i1-u16": (103, 101, 2, 99, 1, np.uint16, (3.3, -2.1), 2.0, 1e-5, 1.2e-5),
    # 1.2e-5 / 5.0e-5
    "301x257-L3-w21-i2-mixed": (301, 257, 3, 21, 2, "mixed", (5.0, 3.0), 3.0, 4e-5, 1.5e-4),
    # 1.1e-4 / 8.2e-4
    "512x512-L4-w15-i3-f32": (512, 512, 4, 15, 3, np.float32, (24.0, -17.0), 2.0, 3.5e-4, 2.5e-3),
    # 5.7e-6 / 9.3e-6
    "130x260-L2-w301-i1-u8": (130, 260, 2, 301, 1, np.uint8, (6.0, -4.0), 2.0, 2e-5, 3e-5),
    # 7.6e-6 / 1.7e-5
    "600x520-L4-w99-i3-u16": (600, 520, 4, 99, 3, np.uint16, (12.5, 7.5), 3.0, 2.5e-5, 5e-5),
    # 8.2e-6 / 2.8e-5
    "256x320-L4-w51-i1-mixed": (256, 320, 4, 51, 1, "mixed", (9.5, -6.25), 2.0, 2.5e-5, 1e-4),
}


@pytest.mark.parametrize("case", list(PYRAMID_CASES))
def test_pyramid_is_the_float64_statement_over_the_whole_image(ref, case):
    H, W, levels, win, iters, dtype, shift, amp, q99, dmax = PYRAMID_CASES[case]
    prev, nxt = moving_pair(H, W, dtype, shift, amp)
    exp = farneback_pyramid_float64(prev, nxt, levels, win, iters)
    for fused in (False, True):
        assert_within(flow_gap(ref.farneback(prev, nxt, levels, win, iters, fused=fused), exp), q99, dmax,
                      f"{case} fused={fused}")


def test_pyramid_with_window_1_is_the_float64_statement_where_it_is_well_posed(ref):
    """Window 1 has no window: each pixel solves its own 2 x 2 system, which is singular where the local quadratic is
    degenerate, and float32 rounding moves those pixels by up to ~50 px here (the flow reaches ~400 px on a 160-px-wide
    image) and, through the next level's initial flow, their neighbours.  No max bound is meaningful; the median and the
    90th percentile are (measured 8.6e-5 / 4.1e-3 px)."""
    prev, nxt = moving_pair(128, 160, np.float32, (4.5, 2.5))
    exp = farneback_pyramid_float64(prev, nxt, 1, 1, 1)
    for fused in (False, True):
        d = flow_gap(ref.farneback(prev, nxt, 1, 1, 1, fused=fused), exp)
        assert np.median(d) <= 5e-4 and np.quantile(d, 0.9) <= 1.5e-2, (np.median(d), np.quantile(d, 0.9))


def test_the_float64_level_table_is_the_restatements(ref):
    for H, W, levels in [(1024, 768, 9), (101, 103, 2), (103, 101, 5), (130, 260, 2), (600, 520, 4), (46000, 3000, 30)]:
        assert level_table(H, W, levels) == ref.level_table(H, W, levels)


# Teeth: each error of PYRAMID_ERRORS, put into the float64 statement, moves it outside the bounds the restatement meets.
# The cases are those of PYRAMID_CASES where every error is separable.  Large windows hide some of them: with window 99
# on 600 x 520, ksize + 2 (outer taps of weight ~1e-5) moves the result by 1.9e-5 px, inside that case's bounds, and with
# window 301 on 130 x 260 a nearest-neighbour flow resize moves it by 3.1e-5 px, at its bound.
TEETH_CASES = ["256x320-L2-w15-i3-f32", "301x257-L3-w21-i2-mixed", "512x512-L4-w15-i3-f32"]


@pytest.fixture(scope="module")
def teeth_flows(ref):
    out = {}
    for case in TEETH_CASES:
        H, W, levels, win, iters, dtype, shift, amp, _, _ = PYRAMID_CASES[case]
        prev, nxt = moving_pair(H, W, dtype, shift, amp)
        out[case] = (prev, nxt, ref.farneback(prev, nxt, levels, win, iters))
    return out


@pytest.mark.parametrize("error", PYRAMID_ERRORS)
@pytest.mark.parametrize("case", TEETH_CASES)
def test_a_convention_error_in_the_float64_statement_is_caught(teeth_flows, case, error):
    H, W, levels, win, iters, _, _, _, q99, dmax = PYRAMID_CASES[case]
    prev, nxt, got = teeth_flows[case]
    d = flow_gap(got, farneback_pyramid_float64(prev, nxt, levels, win, iters, error=error))
    assert np.quantile(d, 0.99) > q99 or d.max() > dmax, (np.quantile(d, 0.99), d.max())


# levels = 0 over the whole image: the restatement is the single-scale oracle, and with OpenCV's border rules the float64
# statement holds in the 5-px attenuation band and where the second image is sampled out of range, which
# tests/test_oracle_independent.py leaves out.  (H, W, win, iterations, dtype, q99 bound, max bound); measured q99 / max
# in the comments, bounds about 3x.
SINGLE_SCALE_CASES = [
    (113, 129, 15, 3, np.float32, 6e-5, 3e-4),     # 1.9e-5 / 1.0e-4
    (129, 113, 15, 3, np.uint8, 6e-5, 2.5e-4),     # 2.1e-5 / 7.1e-5
    (71, 93, 51, 2, np.uint16, 1.5e-5, 2e-5),      # 4.6e-6 / 5.5e-6
    (200, 220, 99, 3, np.float32, 6e-6, 1e-5),     # 1.7e-6 / 3.3e-6
]


@pytest.mark.parametrize("H,W,win,iters,dtype,q99,dmax", SINGLE_SCALE_CASES)
def test_levels_zero_is_the_float64_statement_over_the_whole_image(ref, H, W, win, iters, dtype, q99, dmax):
    prev, nxt = moving_pair(H, W, dtype, (1.3, -0.7))
    exp = farneback_float64(prev, nxt, win, iters, det_eps=1e-3, opencv_borders=True)
    assert np.array_equal(exp, farneback_pyramid_float64(prev, nxt, 0, win, iters))
    for fused in (False, True):
        got = ref.farneback(prev, nxt, 0, win, iters, fused=fused)
        assert_within(flow_gap(got, exp), q99, dmax, f"fused={fused}")
    # without the border rules the band is off by pixels: the rules are what the whole-image bound rests on
    d = flow_gap(got, farneback_float64(prev, nxt, win, iters, det_eps=1e-3))
    assert d.max() > 100 * dmax
