"""The push-pull fill of a flow without a GPU: the numpy float32 statement of include/microaligner_flowfill.h
(tests/_flow_fill_ref.py) held to the same formulas in float64, its properties (kept pixels bit for bit, identity, all
dropped, one kept pixel, the range of the kept values), what it is good for beside smooth_flow (the table of the README),
the argument checks of device.fill_flow_params, and the plumbing of the new header."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_fill_ref as R  # noqa: E402
import _flow_smooth_ref as S  # noqa: E402
from _measured_path import HASH  # noqa: E402
from microaligner_amd import _lib  # noqa: E402
from microaligner_amd.device import FillInfo, fill_flow_params  # noqa: E402

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowfill.h")
SHAPES = [(96, 160), (37, 515), (257, 300)]
K_MEASURED = 3.36          # the largest K of the three cases below (2.78, 3.05, 3.36)
K_ALLOWED = 4 * K_MEASURED


def same_bits(got, exp):
    assert got.dtype == exp.dtype and got.shape == exp.shape
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(got.view(np.uint32)[~gn], exp.view(np.uint32)[~en])


@pytest.mark.parametrize("shape", SHAPES)
def test_float32_statement_against_float64(shape):
    """|float32 - float64| <= K 2^-24 max|f| with K = 4 x 3.36 = 13.44.  Measured over these three cases (a smooth field, a
    rectangular hole half the image wide, 20 % of the pixels dropped at random, 20 % with soft weights): K = 2.78 at
    96 x 160, 3.05 at 37 x 515 and 3.36 at 257 x 300; the bound is four times the largest."""
    f, w = R.holed_case(*shape)
    o32, c32, L = R.fill_flow_ref(f, w)
    o64, c64, L64 = R.fill_flow_ref(f, w, dtype=F64)
    assert o32.dtype == F32 and o64.dtype == F64 and c32 == c64 and L == L64 == (max(shape) - 1).bit_length()
    assert c32[0] > 0.3 * f[..., 0].size and c32[1] > 0.05 * f[..., 0].size and c32[2] == 0
    K = np.abs(o32.astype(F64) - o64).max() / (2.0 ** -24 * np.abs(f).max())
    print(f"{shape}: K = {K:.2f}")
    assert K <= K_ALLOWED


@pytest.mark.parametrize("shape", SHAPES + [(1, 1), (1, 2), (2, 1), (1, 300), (7, 5)])
def test_properties(shape):
    H, W = shape
    f, w = R.holed_case(H, W, 1)
    w[H // 2:, :W // 3] = 1.5                                  # weights above 1 saturate
    w[H - 1, W - 1] = 1.5
    out, counts, L = R.fill_flow_ref(f, w)
    assert same_bits(out[w >= 1], f[w >= 1])                   # pixels of weight >= 1 come back bit for bit
    assert counts[0] == int((w == 0).sum()) and counts[1] == int(((w > 0) & (w < 1)).sum()) and counts[2] == 0
    full, counts, _ = R.fill_flow_ref(f)
    assert same_bits(full, f) and counts == (0, 0, 0)          # nothing dropped: the input
    none, counts, _ = R.fill_flow_ref(f, np.zeros((H, W), np.uint8))
    assert np.isnan(none).all() and counts == (H * W, 0, H * W)
    none, counts, _ = R.fill_flow_ref(np.full((H, W, 2), np.nan, F32))
    assert np.isnan(none).all() and counts == (H * W, 0, H * W)
    one = np.zeros((H, W), np.uint8)
    one[H - 1, W // 3] = 7
    g = f.copy()
    g[H - 1, W // 3] = (2.5, -7.0)
    out, counts, _ = R.fill_flow_ref(g, one)
    assert np.all(out == F32([2.5, -7.0])) and counts == (H * W - 1, 0, 0)
    # cells and masks are the same weight said three ways
    cells = (np.random.default_rng(3).random((-(-H // 16), -(-W // 48))) < 0.7).astype(F32)
    px = np.ascontiguousarray(np.repeat(np.repeat(cells, 16, 0), 48, 1)[:H, :W])
    a = R.fill_flow_ref(f, cells, (16, 48))
    assert same_bits(a[0], R.fill_flow_ref(f, px)[0]) and same_bits(a[0], R.fill_flow_ref(f, (px * 9).astype(np.uint8))[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_output_stays_in_the_range_of_the_kept_values(shape):
    """Every level's mean, interpolation and blend is a convex combination of values already in range, in at most eight
    rounded operations: the output lies within [min, max] of the kept values up to 8 L 2^-24 max|kept| per component."""
    f, w = R.holed_case(*shape, 2)
    out, _, L = R.fill_flow_ref(f, w)
    kept = f[w > 0]
    slack = 8 * L * 2.0 ** -24 * np.abs(kept).max()
    for c in range(2):
        assert kept[:, c].min() - slack <= out[..., c].min() and out[..., c].max() <= kept[:, c].max() + slack


SOFT = F32(1.0 / 16)        # the weight the filled pixels get in the smoothing that follows a fill


def usefulness_rows(diameters=(40, 150, 400), n=512):
    """the table of the README.  Per disc diameter: the endpoint error inside the disc, (mean, max), of fill_flow alone and
    of fill_flow followed by smooth_flow(sigma=4, weight=where(keep, 1, 1 / 16), where="blend") -- the filled pixels keep a
    small weight, so that the smoothing reads them where no kept pixel is near; the pixels smooth_flow(sigma=6,
    where="blend") alone leaves unsupported; the largest jump between a filled pixel and an adjacent kept pixel and the
    flow's own largest slope; and the largest second difference (crease) of the filled flow, of the smoothed one and of the
    flow itself."""
    rows = []
    for d in diameters:
        f, keep, inside = R.disc_case(n, d)
        holed = np.where(inside[..., None], F32(np.nan), f)
        filled, counts, _ = R.fill_flow_ref(holed, keep)
        assert counts == (int(inside.sum()), 0, 0)
        smoothed, left = S.smooth_flow_ref(filled, S.gaussian_taps(4.0), np.where(keep > 0, F32(1), SOFT), None, "blend")
        assert left == 0
        _, unsupported = S.smooth_flow_ref(holed, S.gaussian_taps(6.0), keep, None, "blend")
        epe = lambda g: np.hypot(*np.moveaxis(g.astype(F64) - f, -1, 0))[inside]        # noqa: E731
        crease = lambda g: max(float(np.abs(np.diff(g.astype(F64), 2, axis=a)).max()) for a in (0, 1))   # noqa: E731
        jump = 0.0
        for axis in (0, 1):
            across = np.diff(inside.astype(np.int8), axis=axis) != 0
            jump = max(jump, float(np.abs(np.diff(filled.astype(F64), axis=axis)).max(-1)[across].max()))
        slope = max(float(np.abs(np.diff(f.astype(F64), axis=a)).max()) for a in (0, 1))
        e1, e2 = epe(filled), epe(smoothed)
        rows.append((d, (e1.mean(), e1.max()), (e2.mean(), e2.max()), unsupported, jump, slope,
                     (crease(filled), crease(smoothed), crease(f))))
    return rows


def test_what_the_fill_is_good_for():
    """fill_flow leaves no pixel without a value.  smooth_flow alone (sigma 6: r = 18) leaves every pixel whose 37 x 37
    window lies inside the disc: none at 40 px (the window's corner is 18 sqrt(2) = 25.5 px from its centre, the rim 20),
    the middle at 150 and 400 px.  The error inside the disc is bounded by the flow's change over the image: the fill is
    within the range of the kept values (test_output_stays_in_the_range_of_the_kept_values), a component changes by at most
    slope x 2 n over the n x n image, and the endpoint error is at most sqrt(2) x the larger component's."""
    for d, e1, e2, unsupported, jump, slope, crease in usefulness_rows():
        print(f"disc {d:3d} px: fill {e1[0]:.3f} mean {e1[1]:.3f} max; then smooth {e2[0]:.3f} mean {e2[1]:.3f} max; "
              f"smooth_flow(6) alone leaves {unsupported} unsupported; jump {jump:.4f} px, slope {slope:.4f} px/px; "
              f"crease {crease[0]:.4f} filled, {crease[1]:.4f} smoothed, {crease[2]:.4f} the flow")
        assert (unsupported > 0) == (d / 2 > 18 * np.sqrt(2))
        assert max(e1[1], e2[1]) <= 2 * np.sqrt(2) * slope * 512


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_fill_flow_params_checks_without_a_device():
    f = np.zeros((20, 30, 2), F32)
    assert fill_flow_params(f) == (20, 30, _lib.MA_SMOOTH_WEIGHT_NONE, 1, 1, 5)
    assert fill_flow_params(f, np.ones((20, 30), F32))[2] == _lib.MA_SMOOTH_WEIGHT_F32
    assert fill_flow_params(f, np.ones((20, 30), np.uint8))[2] == _lib.MA_SMOOTH_WEIGHT_U8
    assert fill_flow_params(f, np.ones((3, 2), F32), (8, 16))[2:5] == (_lib.MA_SMOOTH_WEIGHT_CELLS, 8, 16)
    assert fill_flow_params(np.zeros((1, 1, 2), F32))[5] == 0 and fill_flow_params(np.zeros((1, 2, 2), F32))[5] == 1
    assert fill_flow_params(np.zeros((5, 3, 2), F32))[5] == 3
    for kw in (dict(flow=f.astype(F64)), dict(flow=f[..., 0]), dict(flow=np.zeros((0, 4, 2), F32)),
               dict(weight=np.ones((20, 31), F32)), dict(weight=np.ones((20, 30), F64)), dict(weight=[1.0]),
               dict(weight=np.ones((3, 2), F32)), dict(cell_size=8), dict(weight=np.ones((20, 30), F32), cell_size=8),
               dict(weight=np.ones((3, 2), F32), cell_size=0), dict(weight=np.ones((3, 2), F32), cell_size=(8, 16, 2))):
        with pytest.raises(ValueError):
            fill_flow_params(**dict(dict(flow=f), **kw))
    assert FillInfo(1, 2, 3, 4).levels == 4 and FillInfo._fields == ("dropped", "blended", "unsupported", "levels")


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    import microaligner_amd
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_fill_flow"] == sorted(_lib.FLOWFILL_SIGNATURES)
    assert hasattr(lib, "ma_fill_flow")
    proto = re.search(r"\bma_fill_flow\s*\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.FLOWFILL_SIGNATURES["ma_fill_flow"][1]) == 10
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES") and t != "FLOWFILL_SIGNATURES"]
    assert len(others) >= 18 and not any(set(_lib.FLOWFILL_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_flowsmooth.h"' in open(HEADER).read()            # the weight kinds are the smoothing's
    assert {"fill_flow", "FillInfo"} <= set(microaligner_amd.__all__)


def test_the_source_hash_is_the_parents(monkeypatch):
    """build.source_hash() reads the files and flags it read before this source existed"""
    from microaligner_amd import build
    before = build.source_hash()
    assert before == HASH and _lib.source_hash() == before
    assert "flow_fill.hip" in build.SOURCES and "microaligner_flowfill.h" not in " ".join(build.HEADERS)
    own = [os.path.basename(h) for h in build.SOURCE_HEADERS["flow_fill.hip"]]
    assert own == ["microaligner_flowfill.h", "microaligner_flowsmooth.h", "weight_map.h", "call_counts.h"]
    monkeypatch.setattr(build, "SOURCES", [s for s in build.SOURCES if s != "flow_fill.hip"])
    monkeypatch.setattr(build, "SOURCE_HEADERS", {k: v for k, v in build.SOURCE_HEADERS.items() if k != "flow_fill.hip"})
    assert build.source_hash() == before
