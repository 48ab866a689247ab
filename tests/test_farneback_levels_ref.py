"""The CPU restatement of cv2.calcOpticalFlowFarneback with levels > 0 (tests/c_ref/farneback_levels_ref.c): pinned to the
single-scale oracle at levels = 0, its level table and resize checked against their formulas, and the pyramid shown to find
the large motion a single scale misses.  The GPU pyramid is compared with it in test_gpu_farneback_levels.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
