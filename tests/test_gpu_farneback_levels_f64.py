"""farneback(..., pyr_size > 0) on the GPU (ma_farneback_levels) against the independent float64 statement of OpenCV's
pyramid (tests/_f64_ref.py::farneback_pyramid_float64) over the whole image: the cases and bounds of
test_farneback_levels_ref.py, where the CPU restatement meets them, and shapes of the kernels' own geometry (tall and
narrow images, sides just above a multiple of 64 or 256, a 2048 x 2048 image with 4 levels and window 99).  The bit-exact
comparison with the restatement is test_gpu_farneback_levels.py; this one does not depend on the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _f64_ref import farneback_pyramid_float64  # noqa: E402
from test_farneback_levels_ref import PYRAMID_CASES, assert_within, flow_gap, moving_pair  # noqa: E402

from microaligner_amd import farneback  # noqa: E402

pytestmark = pytest.mark.gpu

# (H, W, levels, win, iterations, dtype, shift, amp, q99 bound, max bound); the gaps the restatement (bit-exact to the
# kernels) has on them, q99 / max over both rounding models, in the comments, the bounds about 3x
GEOMETRY_CASES = {
    # 3.5e-4 / 4.5e-3
    "2000x70-L2-w15-i3-u8": (2000, 70, 2, 15, 3, np.uint8, (9.5, -6.25), 2.0, 1e-3, 1.5e-2),
    # 3.9e-4 / 4.0e-3
    "70x2000-L2-w15-i3-f32": (70, 2000, 2, 15, 3, np.float32, (9.5, -6.25), 2.0, 1.2e-3, 1.2e-2),
    # 9.1e-6 / 2.4e-5
    "257x321-L2-w51-i2-f32": (257, 321, 2, 51, 2, np.float32, (9.5, -6.25), 2.0, 3e-5, 7e-5),
    # 4.5e-5 / 3.1e-4
    "513x769-L3-w15-i3-u16": (513, 769, 3, 15, 3, np.uint16, (12.0, 5.0), 2.0, 1.5e-4, 1.2e-3),
    # 3.0e-6 / 5.0e-6
    "65x257-L1-w99-i2-mixed": (65, 257, 1, 99, 2, "mixed", (3.0, 2.0), 2.0, 1e-5, 1.5e-5),
    # 1.4e-5 / 3.7e-5; the float64 side peaks at ~1.5 GB of host memory
    "2048x2048-L4-w99-i2-f32": (2048, 2048, 4, 99, 2, np.float32, (24.0, -17.0), 2.0, 4e-5, 1.2e-4),
}
CASES = {**PYRAMID_CASES, **GEOMETRY_CASES}


@pytest.mark.parametrize("case", list(CASES))
def test_pyramid_kernels_are_the_float64_statement_over_the_whole_image(ctx, case):
    H, W, levels, win, iters, dtype, shift, amp, q99, dmax = CASES[case]
    prev, nxt = moving_pair(H, W, dtype, shift, amp)
    exp = farneback_pyramid_float64(prev, nxt, levels, win, iters)
    dprev, dnxt = ctx.asdevice(prev), ctx.asdevice(nxt)
    for fused in (False, True):
        got = farneback(prev, nxt, pyr_size=levels, win_size=win, num_iter=iters, muladd_fused=fused)
        assert_within(flow_gap(got, exp), q99, dmax, f"{case} farneback() fused={fused}")
        got = ctx.farneback(dprev, dnxt, win, iters, fused=fused, levels=levels).numpy()
        assert_within(flow_gap(got, exp), q99, dmax, f"{case} ctx.farneback() fused={fused}")


def test_pyramid_kernels_with_window_1_are_the_float64_statement_where_it_is_well_posed(ctx):
    # the median / 90th-percentile bounds of test_farneback_levels_ref.py, for the reason given there
    prev, nxt = moving_pair(128, 160, np.float32, (4.5, 2.5))
    exp = farneback_pyramid_float64(prev, nxt, 1, 1, 1)
    for fused in (False, True):
        d = flow_gap(farneback(prev, nxt, pyr_size=1, win_size=1, num_iter=1, muladd_fused=fused), exp)
        assert np.median(d) <= 5e-4 and np.quantile(d, 0.9) <= 1.5e-2, (np.median(d), np.quantile(d, 0.9))
