"""Pyramid Farneback against the REAL OpenCV through tests/golden/cv2_levels_4.5.5.npz (made by
tests/golden/make_cv2_levels_golden.py with numpy + opencv-contrib-python==4.5.5.64).  While the file is absent the tests
SKIP and the restatement's rules stay unpinned.  Bars: resize and GaussianBlur within a few float32 ulp,
flows within FLOW_TOL px in one of the two rounding models (the one the recorded build follows)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_cv2_levels_golden as G  # noqa: E402
from _fb_levels_ref import LevelsRef  # noqa: E402

from oracle import oracle  # noqa: E402

FLOW_TOL = 1e-3   # px
F32_RTOL = 2e-6
SKIP_REASON = ("tests/golden/cv2_levels_4.5.5.npz is absent: run `python tests/golden/make_cv2_levels_golden.py` with numpy "
               "and opencv-contrib-python==4.5.5.64 and commit the file")


@pytest.fixture(scope="module")
def golden():
    if not os.path.exists(G.OUT):
        pytest.skip(SKIP_REASON)
    return dict(np.load(G.OUT))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return LevelsRef(tmp_path_factory.mktemp("fb_levels_ref"))


def _close_in_a_model(fn, exp, tol):
    errs = [float(np.abs(fn(fused) - exp).max()) for fused in (False, True)]
    assert min(errs) <= tol, f"max |diff| unfused {errs[0]}, fused {errs[1]}"


@pytest.mark.parametrize("si", range(len(G.SHAPES)))
def test_resize_and_blur_at_the_level_sizes(golden, ref, si):
    H, W = G.SHAPES[si]
    f = golden[f"s{si}_prev"].astype(np.float32)
    table = G.level_table(H, W, max(G.LEVELS))
    for k, (w, h, ks, sigma) in enumerate(table[1:], start=1):
        np.testing.assert_allclose(ref.resize_linear(f, (w, h)), golden[f"s{si}_resize_k{k}"], rtol=F32_RTOL, atol=1e-4)
        np.testing.assert_allclose(oracle.gaussian_blur(f, ks, sigma), golden[f"s{si}_blur_k{k}"], rtol=F32_RTOL, atol=1e-4)
        up = table[k - 1][:2]
        np.testing.assert_allclose(ref.resize_linear(golden[f"s{si}_field_k{k}"], up), golden[f"s{si}_fieldup_k{k}"],
                                   rtol=F32_RTOL, atol=1e-5)


@pytest.mark.parametrize("si", range(len(G.SHAPES)))
def test_restatement_flow(golden, ref, si):
    prev, nxt = golden[f"s{si}_prev"], golden[f"s{si}_next"]
    for lv in G.LEVELS:
        for win in G.WINS:
            _close_in_a_model(lambda fused: ref.farneback(prev, nxt, lv, win, G.ITERS, fused=fused),
                              golden[f"s{si}_flow_l{lv}_w{win}"], FLOW_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(G.SHAPES)))
def test_hip_flow(golden, si):
    from microaligner_amd import farneback
    prev, nxt = golden[f"s{si}_prev"], golden[f"s{si}_next"]
    for lv in G.LEVELS:
        for win in G.WINS:
            _close_in_a_model(lambda fused: farneback(prev, nxt, pyr_size=lv, win_size=win, num_iter=G.ITERS,
                                                      muladd_fused=fused),
                              golden[f"s{si}_flow_l{lv}_w{win}"], FLOW_TOL)
