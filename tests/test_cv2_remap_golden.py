"""cv2.remap's four interpolation modes against the REAL OpenCV through tests/golden/cv2_remap_4.5.5.npz (made by
tests/golden/make_cv2_remap_golden.py with numpy + opencv-contrib-python==4.5.5.64).  While the file is absent the tests
SKIP and the restatement's nearest / cubic / Lanczos-4 rules stay unpinned against OpenCV.  Bar: bit
for bit (equal NaN masks), on the CPU restatement and, under -m gpu, on the HIP path."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_cv2_remap_golden as G  # noqa: E402
from _remap_interp_ref import InterpRef  # noqa: E402

SKIP_REASON = ("tests/golden/cv2_remap_4.5.5.npz is absent: run `python tests/golden/make_cv2_remap_golden.py` with numpy "
               "and opencv-contrib-python==4.5.5.64 and commit the file")


@pytest.fixture(scope="module")
def golden():
    if not os.path.exists(G.OUT):
        pytest.skip(SKIP_REASON)
    return dict(np.load(G.OUT))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return InterpRef(tmp_path_factory.mktemp("remap_interp_ref_golden"))


def same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp).reshape(np.shape(got))
    assert got.dtype == exp.dtype, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), f"{what}: NaN masks differ"
    bad = ~(np.isnan(got) | (got == exp))
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at {np.argwhere(bad)[:3].tolist()}"


def cases(golden):
    """(name, src, map, mode, expected) of every recorded remap"""
    for dn in G.DTYPES:
        for si in range(len(G.SRC_SHAPES)):
            src = golden[f"{dn}_s{si}_src"]
            for mn in ["subpixel", "integer", "half", "edges", "bad"]:
                m = golden[f"{dn}_s{si}_{mn}_map"]
                for mode in G.MODES:
                    yield f"{dn}_s{si}_{mn}_{mode}", src, m, mode, golden[f"{dn}_s{si}_{mn}_{mode}"]
        for mode in G.KOFF:
            yield f"{dn}_impulse_{mode}", G.impulse_image(dn), G.impulse_map(mode), mode, golden[f"{dn}_impulse_{mode}"]
    for mn in ["subpixel", "integer", "half", "edges", "bad"]:
        for mode in G.MODES:
            yield (f"nonfinite_{mn}_{mode}", golden["nonfinite_src"], golden[f"nonfinite_{mn}_map"], mode,
                   golden[f"nonfinite_{mn}_{mode}"])


def test_restatement_equals_opencv(golden, ref):
    for name, src, m, mode, exp in cases(golden):
        same_bits(ref.remap(src, m, mode), exp, name)


@pytest.mark.gpu
def test_hip_equals_opencv(golden, ctx):
    for name, src, m, mode, exp in cases(golden):
        if mode == "linear" and src.ndim == 3 and src.shape[2] > 2:
            continue   # the linear remap takes 1 or 2 channels
        same_bits(ctx.remap(ctx.asdevice(src), ctx.asdevice(m), interpolation=mode).numpy(), exp, name)
