"""-m gpu: the kernels at the edges of their own geometry, bit for bit against the CPU oracle.

Tiled kernels go wrong where an image is narrower than a stencil, thinner than a border band, one pixel off a block or strip
size, or where a reflect-101 border folds more than once; size checks go wrong one byte either side of a limit.  This file
puts Farneback (untiled, tiled, pyramid), dog() and register() + warp() on such shapes, and pins the one size limit of
whole-window Farneback: a window's 20 float planes (rows padded to 64 floats) are addressed with 32-bit byte offsets, so a
window above INT32_MAX bytes is refused with ValueError before anything is launched (5178 x 5178 is the largest square).
The refusal cases run with the workspace limit at INT32_MAX bytes, so that even a build without the size check refuses them
before any launch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _f64_ref import dog_float64, farneback_float64, shifted_texture_pair  # noqa: E402
from _fb_levels_ref import LevelsRef  # noqa: E402
from conftest import oracle_threads  # noqa: E402

from oracle import oracle as O  # noqa: E402
from oracle import register_oracle as RO  # noqa: E402
from microaligner_amd import _lib as L  # noqa: E402
from microaligner_amd import OptFlowRegistrator, Warper, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


def _pair(h, w, seed, dtype=np.float32):
    return synthetic.make_pair(h, w, seed=seed, dtype=dtype)


def _assert_same(got, exp):
    assert got.shape == exp.shape and got.dtype == exp.dtype
    bad = got != exp
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, max |diff| {np.abs(got - exp).max()}"


@pytest.fixture(autouse=True)
def _oracle_threads():
    # per test: RO.register() sets its own thread count
    O.set_threads(oracle_threads())


# ---- A. untiled Farneback ---------------------------------------------------------------------------------------------
# Sides around the 3x3 expansion, the 5-px border attenuation on both sides, the 64 x 16 tile of fb_polyexp_m0, the 112 x 32
# tile of fb_blur_h_solve, the 56 / 112 rows of the vertical blurs and the 32-column alignment of the needed rectangle;
# windows from m = 0 (the fallback kernels) through every fast-path class to 301 (fallback again), most of them larger
# than the image.  Every pair of factor values occurs (a covering set over all H x W, not the full product).
SIDES = [1, 2, 3, 4, 5, 9, 10, 11, 15, 16, 17, 31, 32, 33, 55, 56, 57, 63, 64, 65, 111, 112, 113, 129]
WINS = [1, 2, 3, 15, 17, 51, 99, 301]
UNTILED = [(h, w, WINS[(i + j) % 8], "u8 u16 f32".split()[(i + 2 * j) % 3], (i + j + (i + j) // 8) % 2 == 1, 1 + (i + j) % 3)
           for i, h in enumerate(SIDES) for j, w in enumerate(SIDES)]
# uint8 rows whose width is not a multiple of 4: the expansion kernel's dword loads start off alignment
UNTILED += [(h, w, win, "u8", fused, 2) for w in range(65, 70) for h, win, fused in ((17, 15, False), (64, 3, True),
                                                                                      (5, 99, False))]


@pytest.mark.parametrize("h,w,win,dt,fused,iters", UNTILED)
def test_untiled_farneback_at_block_edges(ctx, h, w, win, dt, fused, iters):
    ref, mov = _pair(h, w, seed=131 * h + w, dtype=DTYPES[dt])
    exp = O.calc_optical_flow_farneback(mov, ref, win, iters, fused=fused)
    got = ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), win, iters, fused=fused).numpy()
    _assert_same(got, exp)


@pytest.mark.parametrize("shape", [(113, 129), (129, 113)])
def test_untiled_farneback_is_the_float64_normal_equations_in_the_interior(ctx, shape):
    """Beyond the bit-exact oracle: an independent float64 statement of the algorithm (tests/_f64_ref.py) on block-edge
    shapes, away from OpenCV's border band, within the bound the oracle meets (tests/test_oracle_independent.py)."""
    h, w = shape
    win, iters = 15, 3
    prev, nxt = shifted_texture_pair(h, w, h + w, (1.3, -0.7))
    got = ctx.farneback(ctx.asdevice(prev), ctx.asdevice(nxt), win, iters).numpy()
    b = 5 + iters * (win // 2) + 3
    exp = farneback_float64(prev, nxt, win, iters, det_eps=1e-3)
    d = np.abs(got[b:-b, b:-b] - exp[b:-b, b:-b])
    assert d.max() <= 2e-5, f"max |gpu - float64 normal equations| = {d.max():.2e} px"
    assert np.abs(np.median(got[b:-b, b:-b].reshape(-1, 2), axis=0) - (1.3, -0.7)).max() < 0.1


@pytest.mark.parametrize("shape", [(113, 129), (129, 113)])
def test_untiled_farneback_is_the_float64_statement_over_the_whole_image(ctx, shape):
    """The sibling of the interior test on the whole image, border band included: with OpenCV's border rules (the
    out-of-range rule of UpdateMatrices and the 5-px attenuation) the float64 statement holds up to the last pixel.
    Measured on the oracle (bit-exact to the kernels): 99th percentile 1.4e-6 px, max 4.9e-6 px."""
    h, w = shape
    win, iters = 15, 3
    prev, nxt = shifted_texture_pair(h, w, h + w, (1.3, -0.7))
    exp = farneback_float64(prev, nxt, win, iters, det_eps=1e-3, opencv_borders=True)
    for fused in (False, True):
        got = ctx.farneback(ctx.asdevice(prev), ctx.asdevice(nxt), win, iters, fused=fused).numpy()
        d = np.abs(got - exp).max(-1)
        assert np.quantile(d, 0.99) <= 5e-6 and d.max() <= 1.5e-5, \
            f"fused={fused}: 99th percentile {np.quantile(d, 0.99):.2e} px, max {d.max():.2e} px"


# ---- B. tiled Farneback -----------------------------------------------------------------------------------------------
# W, H = k * tile + r: ragged last tiles of 1, 2, 31, 32 and 33 px; overlap 0 (windows of exactly one tile), 1 and a
# regular one
TILED = [(2 * 64 + ry, 3 * 64 + rx, 64, ov, win, DTYPES[dt], fused)
         for (ry, rx, ov, win, dt, fused) in [(1, 33, 0, 1, "f32", False), (2, 32, 0, 15, "u8", True),
                                               (31, 1, 0, 3, "u16", False), (32, 2, 1, 1, "f32", True),
                                               (33, 31, 1, 2, "u8", False), (1, 2, 1, 17, "f32", False),
                                               (31, 32, 20, 19, "u16", True), (33, 1, 20, 19, "f32", False),
                                               (2, 31, 20, 51, "u8", False), (32, 33, 0, 99, "f32", False)]]


@pytest.mark.parametrize("H,W,tile,ov,win,dtype,fused", TILED)
def test_tiled_farneback_ragged_remainders(ctx, H, W, tile, ov, win, dtype, fused):
    ref, mov = _pair(H, W, seed=H * 7 + W, dtype=dtype)
    exp = RO.tile_flow(ref, mov, tile, ov, win, 2, fused=fused)
    got = ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), win, 2, tile=tile, overlap=ov, fused=fused).numpy()
    _assert_same(got, exp)


def test_overlap_zero_is_accepted_as_the_oracle_accepts_it(ctx):
    """The reference slices with any overlap >= 0; so do the oracle and the library: windows of exactly one tile."""
    ref, mov = _pair(150, 140, seed=5)
    exp = RO.tile_flow(ref, mov, 50, 0, 15, 2)
    _assert_same(ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), 15, 2, tile=50, overlap=0).numpy(), exp)
    with pytest.raises(ValueError):
        ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), 15, 2, tile=50, overlap=-1)


# ---- C. pyramid Farneback against the CPU restatement of OpenCV's level loop -------------------------------------------
@pytest.fixture(scope="module")
def lref(tmp_path_factory):
    r = LevelsRef(tmp_path_factory.mktemp("fb_levels_ref_edges"))
    r.set_threads(oracle_threads())
    return r


# sides around 64 and 128 with 1-3 levels: levels that stop at the 32-px minimum or just above it, odd sides whose level
# sizes round half to even (65 -> 32, 129 -> 64), window 99 on a 32-px coarse level, uint8 with both sides even (the 2x
# area fast path of the level images) and with mixed parity
LEVELS = [
    (63, 64, 1, 15, 2, "f32", False),
    (64, 64, 1, 15, 2, "u8", True),
    (65, 63, 1, 3, 3, "u16", False),
    (64, 65, 1, 51, 1, "f32", True),
    (127, 128, 2, 15, 2, "u8", False),
    (128, 128, 2, 99, 3, "f32", False),
    (128, 128, 2, 99, 2, "u8", True),
    (129, 127, 2, 17, 2, "u16", True),
    (128, 129, 3, 15, 1, "u8", False),
    (129, 129, 3, 99, 2, "f32", True),
    (65, 129, 2, 1, 2, "f32", False),
    (128, 64, 3, 2, 2, "u8", False),
    (127, 65, 3, 301, 1, "f32", False),
]


@pytest.mark.parametrize("H,W,levels,win,iters,dt,fused", LEVELS)
def test_pyramid_farneback_small_levels(lref, ctx, H, W, levels, win, iters, dt, fused):
    ref, mov = _pair(H, W, seed=H + 3 * W, dtype=DTYPES[dt])
    exp = lref.farneback(mov, ref, levels, win, iters, fused=fused)
    got = ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), win, iters, levels=levels, fused=fused).numpy()
    _assert_same(got, exp)


def test_pyramid_level_sizes_round_half_to_even(lref):
    assert [(w, h) for w, h, _, _ in lref.level_table(129, 65, 3)] == [(65, 129), (32, 64)]
    assert [(w, h) for w, h, _, _ in lref.level_table(128, 128, 2)] == [(128, 128), (64, 64), (32, 32)]


# ---- D. dog() ---------------------------------------------------------------------------------------------------------
# sides at which the 41-tap reflect-101 border folds more than once (<= 20) and around the kernels' strips and segments
TINY = [1, 2, 3, 19, 20, 21, 40, 41]
DOG_SHAPES = [(h, w) for h in TINY for w in TINY] + [(h, w) for h in (63, 64, 65, 255, 256, 257)
                                                     for w in (63, 64, 65, 127, 128, 129)]


@pytest.mark.parametrize("shape", DOG_SHAPES)
def test_dog_at_small_sides_and_strip_edges(ctx, shape):
    """Both kernel paths -- sigmas 5 / 9 take the fused kernel, 3 / 5 the row and column passes -- in all four rounding
    models, bit for bit the oracle; and within one grey level of the float64 chain (reflect-101 at any fold count), equal
    at all but 1 + n / 2000 pixels (measured: at most 7 of 33 153)."""
    h, w = shape
    i = DOG_SHAPES.index(shape)
    img, _ = _pair(h, w, seed=1000 * h + w, dtype=(np.uint8, np.uint16, np.float32)[i % 3])
    d = ctx.asdevice(img)
    for sigmas in ((5, 9), (3, 5)):
        exp64 = dog_float64(img, *sigmas)
        for flags in (0, O.DOG_FUSED_BLUR, O.DOG_FUSED_SCALE, O.DOG_FUSED):
            exp = O.dog(img, True, *sigmas, flags=flags)
            got = ctx.dog_u8(d, *sigmas, flags=flags).numpy()
            _assert_same(got, exp)
            if np.isnan(exp64).any():          # 1 x 1: both normalisations divide by a zero range
                assert h * w == 1
                continue
            diff = np.abs(got.astype(np.float64) - exp64)
            assert diff.max() <= 1 and (diff > 0).sum() <= 1 + h * w // 2000, (sigmas, flags)


@pytest.mark.parametrize("shape", [(1, 1), (20, 3), (64, 129), (257, 65)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_dog_of_a_constant_image(ctx, shape, dtype):
    img = np.full(shape, 7, dtype)
    for sigmas in ((5, 9), (3, 5)):
        _assert_same(ctx.dog_u8(ctx.asdevice(img), *sigmas).numpy(), O.dog(img, True, *sigmas))


# ---- E. register() + warp() on tiny images ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (7, 150), (150, 7), (99, 99)])
@pytest.mark.parametrize("use_dog", [False, True])
@pytest.mark.parametrize("tile,ov", [(1000, 100), (50, 10)])
def test_register_and_warp_on_tiny_images(shape, use_dog, tile, ov):
    """No pyramid level is kept (every side below 200 px): full resolution only, untiled or tiled."""
    params = dict(num_pyr_lvl=2, use_full_res_img=True, use_dog=use_dog, tile_size=tile, overlap=ov)
    ref, mov = _pair(*shape, seed=sum(shape), dtype=np.uint8)
    exp, reports = RO.register(ref, mov, **params)
    reg = OptFlowRegistrator()
    reg.verbose = False
    for k, v in params.items():
        setattr(reg, k, v)
    reg.ref_img, reg.mov_img = ref, mov
    got = reg.register()
    assert [(r.factor, r.accepted) for r in reg.level_reports] == [(r[0], r[3]) for r in reports] == [(1, reports[0][3])]
    np.testing.assert_allclose([(r.mi_after, r.mi_before) for r in reg.level_reports], [r[1:3] for r in reports],
                               rtol=0, atol=1e-12)
    _assert_same(got, exp)
    w = Warper()
    w.tile_size, w.overlap = tile, ov
    w.image, w.flow = mov, got
    _assert_same(w.warp(), RO.warp(mov, exp, tile, ov))


# ---- F. the window size limit ----------------------------------------------------------------------------------------
def _window_bytes(ph, pw):
    return 20 * ph * (-(-pw // 64) * 64) * 4


def test_limit_arithmetic():
    assert _window_bytes(26214, 1024) == 2147450880 <= INT32_MAX < _window_bytes(26215, 1024)
    assert _window_bytes(16384, 1600) <= INT32_MAX < _window_bytes(16384, 1601)     # the 64-float row pitch decides
    assert _window_bytes(5178, 5178) <= INT32_MAX < _window_bytes(5179, 5179)


@pytest.mark.parametrize("H,W", [(26214, 1024), (16384, 1600)])
def test_largest_untiled_windows_are_bit_exact(ctx, H, W):
    ref, mov = _pair(H, W, seed=H % 97, dtype=np.uint8)
    exp = O.calc_optical_flow_farneback(mov, ref, 15, 2)
    got = ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), 15, 2).numpy()
    _assert_same(got, exp)


def test_largest_square_tiled_window_is_bit_exact(ctx):
    """tile 5000 + 2 x 89 = 5178: one zero-padded window around a small image, against the oracle on that window."""
    ref, mov = _pair(300, 260, seed=9, dtype=np.float32)
    tile, ov = 5000, 89
    rt, grid = RO.split_tiles(ref, tile, ov)
    mt, _ = RO.split_tiles(mov, tile, ov)
    assert grid == (1, 1) and rt[0].shape == (5178, 5178)
    exp = RO.stitch_tiles([O.calc_optical_flow_farneback(mt[0], rt[0], 15, 2)], grid, ref.shape, tile, ov)
    got = ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), 15, 2, tile=tile, overlap=ov).numpy()
    _assert_same(got, exp)


def _refused(ctx, call, match):
    """call() must raise ValueError naming the 32-bit plane limit, with nothing launched, under a workspace limit of
    INT32_MAX bytes; the context then still gives the oracle's result."""
    old = ctx.get_option(L.MA_OPT_WORKSPACE_LIMIT)
    try:
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, INT32_MAX)
        ctx.sync()
        ctx.profile(True)
        ctx.profile_reset()
        with pytest.raises(ValueError, match=match) as e:
            call()
        assert str(INT32_MAX) in str(e.value) and "5178 x 5178" in str(e.value)
        ctx.sync()
        launches = {k: v["launches"] for k, v in ctx.profile_get().items() if v["launches"]}
        assert not launches, f"launched before refusing: {launches}"
    finally:
        ctx.profile(False)
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, old)
    ref, mov = _pair(60, 70, seed=3)
    _assert_same(ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), 15, 2).numpy(),
                 O.calc_optical_flow_farneback(mov, ref, 15, 2))


@pytest.mark.parametrize("H,W", [(26215, 1024), (16384, 1601)])
def test_untiled_window_above_the_limit_is_refused(ctx, H, W):
    img = ctx.asdevice(np.zeros((H, W), np.uint8))
    _refused(ctx, lambda: ctx.farneback(img, img, 15, 2), rf"window of {H} x {W} px too large")


def test_tiled_window_above_the_limit_is_refused(ctx):
    img = ctx.asdevice(np.zeros((300, 260), np.float32))
    _refused(ctx, lambda: ctx.farneback(img, img, 15, 2, tile=5001, overlap=89), "window of 5179 x 5179 px too large")


def test_pyramid_with_every_level_dropped_is_refused_as_the_whole_image(ctx):
    """63 rows: level 1 would be 31.5 rows, below OpenCV's 32 -- the call is the single-scale one on 63 x 430 000."""
    img = ctx.asdevice(np.zeros((63, 430000), np.uint8))
    _refused(ctx, lambda: ctx.farneback(img, img, 15, 2, levels=3), "window of 63 x 430000 px too large")


def test_pyramid_above_the_limit_is_refused(ctx):
    img = ctx.asdevice(np.zeros((5200, 5200), np.uint8))
    _refused(ctx, lambda: ctx.farneback(img, img, 15, 2, levels=2), "window of 5200 x 5200 px too large")


def test_register_refuses_a_tile_size_that_leaves_a_level_untiled_above_the_limit(ctx):
    """tile_size 3000 on 5200^2: 5200 / 3000 < 2, so the full-resolution level is one whole 5200^2 window.  Refused before
    the pyramid is built."""
    img = np.zeros((5200, 5200), np.uint8)
    reg = OptFlowRegistrator()
    reg.verbose = False
    reg.num_pyr_lvl, reg.use_full_res_img, reg.tile_size, reg.overlap = 1, True, 3000, 100
    reg.ref_img, reg.mov_img = img, img
    _refused(ctx, reg.register, "tile_size=3000.* one whole window of 5200 x 5200 px")


@pytest.mark.parametrize("win,iters", [(1, 2), (301, 1)])
def test_untiled_fallback_kernels_on_more_rows_than_the_grid_limit(ctx, win, iters):
    """Windows 1 and 301 take the per-pixel fallback kernels, which put rows on the grid's y axis (65 535 at most)."""
    ref, mov = _pair(66000, 64, seed=win, dtype=np.uint8)
    exp = O.calc_optical_flow_farneback(mov, ref, win, iters)
    got = ctx.farneback(ctx.asdevice(mov), ctx.asdevice(ref), win, iters).numpy()
    _assert_same(got, exp)
    assert np.abs(got[65535:]).max() > 0
