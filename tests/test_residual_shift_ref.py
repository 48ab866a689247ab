"""Residual shift maps on the CPU (no GPU): the numpy statement of include/microaligner_residual.h
(tests/_residual_shift_ref.py) against a brute-force evaluation with Python integers, its tie rule and at_limit flag, its
sub-pixel accuracy against analytically shifted textures, its reading of the synthetic pair the GPU end-to-end test uses,
argument validation before any device work, and the C-ABI of the header against the built library and
_lib.RESIDUAL_SIGNATURES."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from _residual_shift_ref import domain, peak, residual_shift_ref, score_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_residual.h")
# What build.source_hash() covered before this feature existed: the sources of the measured path, then build.HEADERS, then
# the compiler flags.  Hashing exactly these again gives the value the commit before the feature gives for the same files
# (cea30b31f12b99d8 on both sides when the feature went in); a literal here would break with every change of a kernel.
MEASURED_PATH_SOURCES = ["ma_api.hip", "farneback.hip", "remap.hip", "pyramid.hip", "dog.hip", "nmi.hip", "register.hip"]

# the pair of the GPU end-to-end test (tests/test_gpu_residual_shift.py) and the R both use
E2E_SHAPE, E2E_SEED, E2E_CELL, E2E_R = (1000, 1200), 4, 250, 6


# ---- brute force -------------------------------------------------------------------------------------------------
def brute_table(a, b, bounds, R):
    """score(d) of one cell from Python integers (unbounded) and math.sqrt; None where the definition gives NaN."""
    h, w = a.shape
    y0, y1, x0, x1 = bounds
    ys = [y for y in range(y0, y1) if R <= y < h - R]
    xs = [x for x in range(x0, x1) if R <= x < w - R]
    al, bl = a.tolist(), b.tolist()
    n = len(ys) * len(xs)
    S_a = sum(al[y][x] for y in ys for x in xs)
    S_aa = sum(al[y][x] ** 2 for y in ys for x in xs)
    va = n * S_aa - S_a * S_a
    out = {}
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            S_b = sum(bl[y + dy][x + dx] for y in ys for x in xs)
            S_bb = sum(bl[y + dy][x + dx] ** 2 for y in ys for x in xs)
            S_ab = sum(al[y][x] * bl[y + dy][x + dx] for y in ys for x in xs)
            num, vb = n * S_ab - S_a * S_b, n * S_bb - S_b * S_b
            out[dy, dx] = None if va == 0 or vb == 0 else float(num) / (math.sqrt(float(va)) * math.sqrt(float(vb)))
    return out


def assert_statement_equals_brute_force(a, b, cell, R):
    from microaligner_amd.shared_modules.registration_qc import cell_bounds
    out = residual_shift_ref(a, b, cell, R)
    bounds = cell_bounds(a.shape, cell)
    for i in range(bounds.shape[0]):
        for j in range(bounds.shape[1]):
            bt = brute_table(a, b, [int(v) for v in bounds[i, j]], R)
            for (dy, dx), v in bt.items():
                got = out["table"][i, j, dy + R, dx + R]
                assert (np.isnan(got) if v is None else got == v), (i, j, dy, dx, got, v)
            finite = {k: v for k, v in bt.items() if v is not None}
            if not finite:
                assert not out["valid"][i, j] and not out["at_limit"][i, j]
                assert np.isnan(out["shift_x"][i, j]) and np.isnan(out["shift_y"][i, j]) and np.isnan(out["score"][i, j])
                continue
            dy, dx = min(finite, key=lambda k: (-finite[k], k[1] ** 2 + k[0] ** 2, k[0], k[1]))
            assert out["valid"][i, j] and out["score"][i, j] == finite[dy, dx]
            assert out["at_limit"][i, j] == (abs(dx) == R or abs(dy) == R)
            assert abs(out["shift_x"][i, j] - dx) <= 0.5 and abs(out["shift_y"][i, j] - dy) <= 0.5
            if bt[0, 0] is not None:
                assert out["score0"][i, j] == bt[0, 0]
    return out


def test_statement_equals_brute_force_on_tiny_inputs():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (23, 19), dtype=np.uint8)
    b = np.roll(a, (1, -2), axis=(0, 1))
    b[rng.random(b.shape) < 0.2] = 0
    assert_statement_equals_brute_force(a, b, (9, 7), 2)          # ragged last row and column of cells
    assert_statement_equals_brute_force(a, b, 30, 3)              # one cell larger than the image
    assert_statement_equals_brute_force(a, b, (1, 19), 1)         # row cells; the first and last have no domain
    assert_statement_equals_brute_force(a, b, (23, 1), 1)         # column cells
    # h or w barely above 2R: a domain of one row / one column / one pixel
    for shape, R in (((7, 15), 3), ((15, 7), 3), ((7, 7), 3), ((3, 9), 1)):
        a2 = rng.integers(0, 256, shape, dtype=np.uint8)
        b2 = rng.integers(0, 256, shape, dtype=np.uint8)
        out = assert_statement_equals_brute_force(a2, b2, 100, R)
        if shape == (7, 7):
            assert not out["valid"].any()                         # one pixel: va = 0
    # h <= 2R: no domain at all
    out = residual_shift_ref(a[:4], b[:4], 8, 2)
    assert not out["valid"].any() and np.isnan(out["table"]).all()


def test_constant_cells_are_invalid_and_partly_constant_cells_are_not():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (24, 36), dtype=np.uint8)
    b = rng.integers(0, 256, (24, 36), dtype=np.uint8)
    a[:12, :12] = 9                      # cell (0, 0): the reference constant -> every score NaN
    b[:13, 10:26] = 200                  # cell (0, 1): b constant on its domain moved by dy <= 1, not by dy = 2
    out = assert_statement_equals_brute_force(a, b, 12, 2)
    assert not out["valid"][0, 0] and np.isnan(out["table"][0, 0]).all() and np.isnan(out["score0"][0, 0])
    t = out["table"][0, 1]
    assert np.isnan(t[2, 2]) and np.isfinite(t).any() and out["valid"][0, 1] and np.isnan(out["score0"][0, 1])
    assert out["valid"][1:].all()


# ---- tie rule and at_limit ---------------------------------------------------------------------------------------------
def test_tie_rule():
    R = 2
    t = np.full((5, 5), 0.25)
    assert peak(t, R) == (0.0, 0.0, 0.25, 0, 1)                  # all equal: the smallest dx^2 + dy^2
    t[2, 2] = np.nan
    assert peak(t, R)[:2] == (0.0, -1.0)                          # distance 1 four times: the smallest dy
    t[1, 2] = np.nan
    assert peak(t, R)[:2] == (-1.0, 0.0)                          # (dx, dy) = (-1, 0) and (1, 0) at dy = 0: the smallest dx
    t[:] = np.nan
    t[0, 4] = -0.5
    assert peak(t, R) == (2.0, -2.0, -0.5, 1, 1)                  # a single finite score on the border
    t[:] = np.nan
    sx, sy, s, lim, ok = peak(t, R)
    assert np.isnan(sx) and np.isnan(sy) and np.isnan(s) and (lim, ok) == (0, 0)
    # refinement: a parabola through (-1, 0.5), (0, 0.9), (1, 0.7) along x peaks at 0.5 * (0.5 - 0.7) / (0.5 - 1.8 + 0.7)
    t[:] = np.nan
    t[2, 1:4] = (0.5, 0.9, 0.7)
    sx, sy, s, lim, ok = peak(t, R)
    assert sx == 0.5 * (0.5 - 0.7) / (0.5 - 2.0 * 0.9 + 0.7) and sy == 0.0 and s == 0.9 and (lim, ok) == (0, 1)


def test_whole_pixel_shifts_come_back_exactly_and_a_larger_shift_sets_at_limit():
    rng = np.random.default_rng(3)
    R = 4
    big = rng.integers(0, 256, (140, 150), dtype=np.uint8)
    a = np.ascontiguousarray(big[20:120, 20:130])
    exact = 0
    for dx, dy in ((0, 0), (1, 0), (0, -1), (3, -2), (-4, 4), (2, 3)):
        b = np.ascontiguousarray(big[20 - dy:120 - dy, 20 - dx:130 - dx])     # b(p + d) = a(p)
        out = residual_shift_ref(a, b, 50, R)
        assert out["valid"].all()
        # The integer peak is the shift exactly.  There num = va = vb as integers, so the score is v / (sqrt(v) * sqrt(v))
        # in float64: two square roots, a product and a quotient, each within 2^-53 relative, so the score is 1.0 to within
        # 4 * 2^-53 -- 1.0 itself in some cells, 1 - 2^-53 or 1 + 2^-52 where sqrt(v)^2 does not round back to v (12 of the
        # 36 cells below give 1.0 exactly).  The parabola then reads the two neighbours of the peak, which nothing makes
        # equal (the windows of b differ), so the refined value is the whole shift to within the sub-pixel bound, and
        # exactly where the axis sits at +-R, which is not refined.
        t = out["table"].reshape(-1, 2 * R + 1, 2 * R + 1)
        assert all(np.unravel_index(int(np.argmax(c)), c.shape) == (dy + R, dx + R) for c in t), (dx, dy)
        exact += int((out["score"] == 1.0).sum())
        assert np.abs(out["score"] - 1.0).max() <= 4 * 2.0 ** -53, (dx, dy)
        assert (np.rint(out["shift_x"]) == dx).all() and (np.rint(out["shift_y"]) == dy).all(), (dx, dy)
        assert np.abs(out["shift_x"] - dx).max() <= 0.05 and np.abs(out["shift_y"] - dy).max() <= 0.05, (dx, dy)
        if abs(dx) == R:
            assert (out["shift_x"] == dx).all()
        if abs(dy) == R:
            assert (out["shift_y"] == dy).all()
        assert (out["at_limit"] == (abs(dx) == R or abs(dy) == R)).all()
        if (dx, dy) == (0, 0):
            assert np.array_equal(out["score0"], out["score"])
    print(f"cells with a score of exactly 1.0: {exact} of 36")
    # a shift of R + 2 along x on a smooth texture: the search runs into the border of the square
    from scipy.ndimage import gaussian_filter
    tex = gaussian_filter(rng.standard_normal((140, 150)), 3.0)
    tex = np.rint((tex - tex.min()) * (255.0 / (tex.max() - tex.min()))).astype(np.uint8)
    a = np.ascontiguousarray(tex[20:120, 20:130])
    b = np.ascontiguousarray(tex[20:120, 20 - (R + 2):130 - (R + 2)])
    out = residual_shift_ref(a, b, 50, R)
    assert out["valid"].all() and out["at_limit"].all() and (out["shift_x"] == R).all()


# ---- sub-pixel accuracy against analytic truth -----------------------------------------------------------------------------
SUBPIXEL_SHIFTS = [(0.0, 0.0), (0.5, 0.5), (1.25, -0.75), (2.0, -3.0), (-2.6, 1.3), (3.3, 3.7), (4.9, -4.1)]   # (dx, dy)


def subpixel_errors(seed=5, size=408, R=6):
    """[(sigma, (dx, dy), error of the estimate, error of the integer peak)] over Gaussian textures of sigma 1.5, 2.5
    and 4 px rounded to u8, the second image the cubic-spline interpolant of the first texture shifted by (dx, dy)."""
    from scipy.ndimage import gaussian_filter, shift as spline_shift
    rng = np.random.default_rng(seed)
    rows = []
    for sigma in (1.5, 2.5, 4.0):
        tex = gaussian_filter(rng.standard_normal((size, size)), sigma, mode="wrap")
        tex = (tex - tex.min()) * (255.0 / (tex.max() - tex.min()))
        a = np.rint(tex).astype(np.uint8)
        for dx, dy in SUBPIXEL_SHIFTS:
            moved = spline_shift(tex, (dy, dx), order=3, mode="grid-wrap")      # moved(p + d) = tex(p)
            b = np.clip(np.rint(moved), 0, 255).astype(np.uint8)
            out = residual_shift_ref(a, b, size, R)
            assert out["valid"][0, 0] and not out["at_limit"][0, 0]
            est = math.hypot(out["shift_x"][0, 0] - dx, out["shift_y"][0, 0] - dy)
            t = out["table"][0, 0]
            iy, ix = np.unravel_index(int(np.nanargmax(t)), t.shape)
            rows.append((sigma, (dx, dy), est, math.hypot(ix - R - dx, iy - R - dy)))
    return rows


def test_subpixel_estimate_against_analytic_shifts():
    """One cell of 408^2, R = 6, 3 textures x 7 shifts.  Bound: 0.05 px, four times the 0.0125 px measured with a numpy
    statement of this definition when the estimator was proposed.  Worst error measured here: 0.0161 px."""
    rows = subpixel_errors()
    worst = max(r[2] for r in rows)
    print(f"worst sub-pixel error over {len(rows)} cases: {worst:.4f} px")
    for sigma, (dx, dy), est, integer in rows:
        print(f"sigma {sigma} shift ({dx}, {dy}): estimate off by {est:.4f} px, integer peak by {integer:.4f} px")
        assert est <= 0.05, (sigma, dx, dy, est)
        if dx != round(dx) or dy != round(dy):
            assert est < integer, (sigma, dx, dy, est, integer)
        else:
            assert est <= 0.05 and integer == 0.0


def e2e_expected_before():
    """-(cell mean of synthetic.displacement()), which holds GLOBAL_SHIFT: make_pair() gives mov(p) = ref(p + d(p)), so
    ref(p) ~ mov(p - d) and, with the header's sign ref(p) ~ mov(p + shift), the shift of the unwarped image is -d."""
    from microaligner_amd import synthetic
    from microaligner_amd.shared_modules.registration_qc import cell_bounds
    H, W = E2E_SHAPE
    dx, dy = synthetic.displacement(H, W, dtype=np.float64)
    dx, dy = np.broadcast_to(dx, (H, W)), np.broadcast_to(dy, (H, W))
    b = cell_bounds((H, W), E2E_CELL)
    ex = np.array([[dx[y0:y1, x0:x1].mean() for (y0, y1, x0, x1) in row] for row in b])
    ey = np.array([[dy[y0:y1, x0:x1].mean() for (y0, y1, x0, x1) in row] for row in b])
    return -ex, -ey


def test_statement_reads_the_synthetic_displacement_at_the_end_to_end_r():
    """The GPU end-to-end test holds `before` to the synthetic displacement within 0.25 px at R = 6 (|d| <= 5.3 px per axis,
    cell means below 5.2): the statement alone meets that here, on the same u8 pair, with no cell at the limit."""
    from microaligner_amd import synthetic
    ref, mov = synthetic.make_pair(*E2E_SHAPE, E2E_SEED, dtype=np.uint8)
    out = residual_shift_ref(ref, mov, E2E_CELL, E2E_R)
    ex, ey = e2e_expected_before()
    assert out["valid"].all() and not out["at_limit"].any()
    ea, eb = np.abs(out["shift_x"] - ex).max(), np.abs(out["shift_y"] - ey).max()
    print(f"statement vs synthetic displacement: worst |dx| error {ea:.3f}, |dy| error {eb:.3f} px")
    assert ea <= 0.25 and eb <= 0.25


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_arguments_are_validated_before_the_device(monkeypatch):
    from microaligner_amd.shared_modules import residual_shift as RS

    def no_device(*a, **k):
        raise AssertionError("validation must not reach the device")
    monkeypatch.setattr(RS, "get_context", no_device)
    ref = np.zeros((40, 30), np.float32)
    flow = np.zeros((40, 30, 2), np.float32)
    bad = [
        dict(mov_img=np.zeros((40, 31), np.float32)),                  # shape mismatch
        dict(mov_img=np.zeros((40, 30), np.int32)),                     # image dtype
        dict(flow=np.zeros((40, 30, 2), np.float64)),                   # flow dtype
        dict(flow=np.zeros((40, 31, 2), np.float32)),                   # flow of another shape
        dict(warped=np.zeros((41, 30), np.float32)),
        dict(cell_size=0), dict(cell_size=(10, 0)), dict(cell_size=(1, 2, 3)),
        dict(labels="raw"),
        dict(max_shift=0), dict(max_shift=17), dict(max_shift=-1), dict(max_shift=2.5), dict(max_shift=True),
        dict(max_shift=15),                                             # w = 30 <= 2R
        dict(tile_size=0), dict(overlap=-1),
    ]
    for kw in bad:
        args = dict(ref_img=ref, mov_img=ref, flow=flow)
        args.update(kw)
        with pytest.raises(ValueError):
            RS.residual_shift(**args)
    with pytest.raises(ValueError):                                     # a side of exactly 2R
        RS.residual_shift(np.zeros((8, 40), np.uint8), np.zeros((8, 40), np.uint8), None, max_shift=4)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (4096, 4096), (0, 0))      # no memory behind it
    with pytest.raises(ValueError):                                     # one cell of 2^24 px > 2^23
        RS.residual_shift(big, big, None, cell_size=4096)
    big2 = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (2049, 4096), (0, 0))
    with pytest.raises(ValueError):                                     # 2^23 + 4096 px
        RS.residual_shift(big2, big2, None, cell_size=(2049, 4096))
    with pytest.raises(AssertionError):                                 # 2^23 exactly passes the checks
        RS.residual_shift(big, big, None, cell_size=(2048, 4096))


def test_null_and_range_arguments_return_einval_without_a_device():
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    f = lib.ma_residual_shift_grid
    d, u = (C.c_double * 64)(), (C.c_ubyte * 64)()
    pd, pu = C.cast(d, C.POINTER(C.c_double)), C.cast(u, C.POINTER(C.c_ubyte))
    img = C.c_void_p(0x1000)      # never dereferenced: every call below fails its checks
    outs = [pd, pd, pd, pd, pu, pu, None]
    good = dict(ctx=C.c_void_p(0x1000), ref=img, b0=img, b1=None, h=40, w=30, ch=10, cw=10, R=4)

    def call(outs0=outs, outs1=(None,) * 7, **kw):
        a = dict(good)
        a.update(kw)
        return f(a["ctx"], a["ref"], a["b0"], a["b1"], a["h"], a["w"], a["ch"], a["cw"], a["R"], *outs0, *outs1)
    assert call(ctx=None) == _lib.MA_EINVAL
    assert b"NULL" in lib.ma_last_error()
    assert call(ref=None) == _lib.MA_EINVAL and call(b0=None) == _lib.MA_EINVAL
    for k in range(6):                                                  # every required output of the first image
        o = list(outs)
        o[k] = None
        assert call(outs0=o) == _lib.MA_EINVAL, k
    assert call(b1=img) == _lib.MA_EINVAL                               # b1 given, its outputs missing
    for R in (0, -1, 17, 1 << 20):
        assert call(R=R) == _lib.MA_EINVAL, R
    assert b"max_shift" in lib.ma_last_error()
    assert call(h=0) == _lib.MA_EINVAL and call(w=0) == _lib.MA_EINVAL and call(h=-5) == _lib.MA_EINVAL
    assert call(ch=0) == _lib.MA_EINVAL and call(cw=-1) == _lib.MA_EINVAL
    assert call(h=4096, w=4096, ch=4096, cw=4096) == _lib.MA_EINVAL     # a cell of 2^24 px
    assert b"2^23" in lib.ma_last_error()


# ---- header, library, bindings, hash ---------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text))), text


def test_residual_header_library_and_bindings_agree():
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    names, text = _declared(HEADER)
    assert names == ["ma_residual_shift_grid"]
    assert hasattr(lib, "ma_residual_shift_grid"), "declared in microaligner_residual.h but not exported"
    assert sorted(_lib.RESIDUAL_SIGNATURES) == names, "ctypes prototypes out of sync with microaligner_residual.h"
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES,
              _lib.FLOWCOMPOSE_SIGNATURES, _lib.FLOWINVERT_SIGNATURES]
    assert not any(set(_lib.RESIDUAL_SIGNATURES) & set(t) for t in others)
    proto = re.search(r"\bma_residual_shift_grid\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    params = [p.strip() for p in proto.split(",")]
    restype, argtypes = _lib.RESIDUAL_SIGNATURES["ma_residual_shift_grid"]
    assert restype is C.c_int and len(params) == len(argtypes) == 23
    for p, t in zip(params, argtypes):
        if p.startswith("double*"):
            assert t is C.POINTER(C.c_double), p
        elif p.startswith("uint8_t*"):
            assert t is C.POINTER(C.c_ubyte), p
        elif p.startswith("int "):
            assert t is C.c_int, p
        else:
            assert t is C.c_void_p, p
    assert '#include "microaligner_hip.h"' in open(HEADER).read()
    assert re.search(r"#define\s+MA_RESIDUAL_MAX_SHIFT\s+16\b", text) and _lib.MA_RESIDUAL_MAX_SHIFT == 16
    assert _lib.MA_RESIDUAL_MAX_CELL_PIXELS == 1 << 23
    # microaligner_qc.h keeps exactly its two declarations
    assert _declared(os.path.join(ROOT, "include", "microaligner_qc.h"))[0] == ["ma_qc_flow_grid", "ma_qc_nmi_grid"]
    import microaligner_amd
    assert callable(microaligner_amd.residual_shift) and "residual_shift" in microaligner_amd.__all__


def test_residual_shift_stays_out_of_the_measured_path_hash(tmp_path, monkeypatch):
    """As test_quality_maps_stay_out_of_the_measured_path_hash: an edit of residual_shift.hip leaves build.source_hash()
    as it is, an edit of dog.hip changes it; and the hash is what the commit without the feature computes."""
    from microaligner_amd import build
    assert "residual_shift.hip" in build.SOURCES and HEADER not in [os.path.abspath(h) for h in build.HEADERS]
    # its own headers: the public one and the cell grid it shares with qc.hip, neither among the hashed ones
    own = [os.path.abspath(h) for h in build.SOURCE_HEADERS["residual_shift.hip"]]
    assert own == [HEADER, os.path.join(build.CSRC, "cell_grid.h")]
    assert not set(own) & {os.path.abspath(h) for h in build.HEADERS}
    out = subprocess.run([sys.executable, "-c", "from microaligner_amd import build; print(build.source_hash())"], cwd=ROOT,
                         capture_output=True, text=True, check=True).stdout.strip()
    assert out == build.source_hash() and re.fullmatch(r"[0-9a-f]{16}", out)
    import hashlib
    hh = hashlib.sha256()
    for path in [os.path.join(build.CSRC, s) for s in MEASURED_PATH_SOURCES] + build.HEADERS:
        hh.update(open(path, "rb").read())
    hh.update(" ".join(build._flags()).encode())
    print(f"build.source_hash() = {out}, without the feature = {hh.hexdigest()[:16]}")
    assert out == hh.hexdigest()[:16]
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc)
    headers = [str((csrc if os.path.samefile(os.path.dirname(h), build.CSRC) else tmp_path) / os.path.basename(h))
               for h in build.HEADERS]
    shutil.copy(os.path.join(ROOT, "include", "microaligner_hip.h"), tmp_path / "microaligner_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADERS", headers)
    assert build.source_hash() == out
    with open(csrc / "residual_shift.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() == out
    with open(csrc / "dog.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() != out
