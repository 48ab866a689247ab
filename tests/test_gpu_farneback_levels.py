"""farneback(..., pyr_size > 0) on the GPU (ma_farneback_levels): bit for bit the CPU restatement of OpenCV's pyramid
(tests/c_ref/farneback_levels_ref.c) in both rounding models, for every input kind, non-finite pixels included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _fb_levels_ref import LevelsRef  # noqa: E402
from conftest import oracle_threads  # noqa: E402

from microaligner_amd import _lib as L  # noqa: E402
from microaligner_amd import farneback, synthetic  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    r = LevelsRef(tmp_path_factory.mktemp("fb_levels_ref"))
    r.set_threads(oracle_threads())
    return r


def _pair(H, W, dtype, seed=11, shift=(9.5, -6.25)):
    a, b = synthetic.make_pair(H, W, seed=seed, shift=shift)
    conv = {np.uint8: lambda x: (np.clip(x, 0, 1) * 255).astype(np.uint8),
            np.uint16: lambda x: (np.clip(x, 0, 1) * 65535).astype(np.uint16),
            np.float32: lambda x: x.astype(np.float32)}
    if dtype == "mixed":
        return conv[np.uint8](a), conv[np.float32](b)
    return conv[dtype](a), conv[dtype](b)


def _same(got, exp):
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    bad = ~((got == exp) | (np.isnan(got) & np.isnan(exp)))
    assert not bad.any(), f"{int(bad.sum())} values differ, max |diff| {np.nanmax(np.abs(got - exp))}"


# (H, W, levels, win, iterations, dtype, fused): every level count, window, iteration count, input kind and rounding
# model, on odd, even and mixed-parity sizes (the 2x area fast path at level 1 needs both sides even)
CASES = [
    (517, 611, 1, 15, 1, np.uint8, False),
    (517, 611, 2, 51, 3, np.uint16, True),
    (517, 611, 3, 99, 1, np.float32, False),
    (517, 611, 4, 15, 3, "mixed", True),
    (1024, 768, 1, 51, 1, np.float32, True),
    (1024, 768, 2, 15, 3, np.uint8, False),
    (1024, 768, 3, 51, 3, np.float32, False),
    (1024, 768, 4, 99, 3, np.uint16, True),
    (1200, 1100, 1, 99, 3, np.uint8, True),
    (1200, 1100, 2, 99, 1, "mixed", False),
    (1200, 1100, 3, 15, 1, np.uint16, False),
    (1200, 1100, 4, 51, 1, np.float32, True),
    (4096, 4096, 4, 99, 3, np.float32, False),
]


@pytest.mark.parametrize("H,W,levels,win,iters,dtype,fused", CASES)
def test_pyramid_matches_the_restatement(ref, H, W, levels, win, iters, dtype, fused):
    mov, refimg = _pair(H, W, dtype)
    got = farneback(mov, refimg, pyr_size=levels, win_size=win, num_iter=iters, muladd_fused=fused)
    exp = ref.farneback(mov, refimg, levels, win, iters, fused=fused)
    _same(got, exp)


def test_levels_zero_is_the_single_scale_entry(ctx):
    mov, refimg = _pair(300, 331, np.float32)
    prev, nxt = ctx.asdevice(mov), ctx.asdevice(refimg)
    exp = ctx.farneback(prev, nxt, 51, 2).numpy()
    flow = ctx.empty((300, 331, 2), np.float32)
    ctx._run(ctx.lib.ma_farneback_levels, prev.ptr, nxt.ptr, L.MA_F32, 300, 331, 0, 0.5, 51, 2, 1, 1.7, 0, flow.ptr)
    assert np.array_equal(flow.numpy(), exp)


def test_levels_beyond_the_minimum_size_are_dropped(ref):
    mov, refimg = _pair(300, 260, np.uint8)
    kept = len(ref.level_table(300, 260, 9)) - 1
    assert kept == 3
    got = farneback(mov, refimg, pyr_size=9, win_size=15, num_iter=2)
    assert np.array_equal(got, farneback(mov, refimg, pyr_size=kept, win_size=15, num_iter=2))
    _same(got, ref.farneback(mov, refimg, 9, 15, 2))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, 1e30])
def test_non_finite_pixels(ref, value):
    mov, refimg = _pair(600, 560, np.float32)
    mov = mov.copy()
    mov[0, 0] = value                 # corner
    mov[3, 300] = value               # inside the reflect-101 radius of the level-4 blur (39 taps) at the top border
    mov[331, 207] = value             # interior
    refimg = refimg.copy()
    refimg[598, 555] = value
    for fused in (False, True):
        got = farneback(mov, refimg, pyr_size=4, win_size=15, num_iter=2, muladd_fused=fused)
        _same(got, ref.farneback(mov, refimg, 4, 15, 2, fused=fused))


def test_device_arrays_in_device_array_out(ctx):
    mov, refimg = _pair(517, 611, np.uint16)
    host = farneback(mov, refimg, pyr_size=3, win_size=51, num_iter=2)
    dev = farneback(ctx.asdevice(mov), ctx.asdevice(refimg), pyr_size=3, win_size=51, num_iter=2)
    assert isinstance(dev, DeviceArray)
    assert np.array_equal(dev.numpy(), host)


def test_a_workspace_limit_below_the_finest_level_raises(ctx):
    mov, refimg = _pair(517, 611, np.float32)
    prev, nxt = ctx.asdevice(mov), ctx.asdevice(refimg)
    old = ctx.get_option(L.MA_OPT_WORKSPACE_LIMIT)
    try:
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, 517 * 640 * 4 * 20 - 1)
        with pytest.raises(ValueError, match="does not fit the workspace limit"):
            ctx.farneback(prev, nxt, 15, 1, levels=2)
    finally:
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, old)
    assert np.array_equal(ctx.farneback(prev, nxt, 15, 1, levels=2).numpy(), farneback(mov, refimg, pyr_size=2, win_size=15))


def test_argument_errors(ctx):
    mov, refimg = _pair(200, 210, np.uint8)
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError):
            farneback(mov, refimg, pyr_size=bad)
    prev, nxt = ctx.asdevice(mov), ctx.asdevice(refimg)
    with pytest.raises(ValueError, match="tile"):
        ctx.farneback(prev, nxt, 15, 1, tile=100, overlap=10, levels=2)
    with pytest.raises(ValueError, match="poly_n"):
        ctx.farneback(prev, nxt, 15, 1, poly_n=3, levels=2)
    flow = ctx.empty((200, 210, 2), np.float32)
    rc = ctx.lib.ma_farneback_levels(ctx.handle, prev.ptr, nxt.ptr, L.MA_U8, 200, 210, 2, C.c_double(0.8), 15, 1, 1, 1.7,
                                     0, flow.ptr)
    assert rc == L.MA_EINVAL and b"pyr_scale" in ctx.lib.ma_last_error()
