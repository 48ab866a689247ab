"""Registration quality maps (assess_registration / flow_qc, include/microaligner_qc.h, csrc/qc.hip).

CPU: cell geometry, argument validation before any device work, the header <-> library <-> bindings agreement, and the
measured path's source hash.  GPU: the per-cell NMI against the gate's kernel on crops (bit for bit) and scikit-learn,
NCC against numpy.corrcoef, the flow statistics against numpy.gradient, agreement with register()'s own gate, and
invariance under input kind, batching and repetition."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QC_HEADER = os.path.join(ROOT, "include", "microaligner_qc.h")


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_cell_bounds_ragged_grid():
    from microaligner_amd.shared_modules.registration_qc import cell_bounds
    b = cell_bounds((2100, 1337), 500)
    assert b.shape == (5, 3, 4) and b.dtype == np.int64
    assert b[0, 0].tolist() == [0, 500, 0, 500]
    assert b[4, 2].tolist() == [2000, 2100, 1000, 1337]
    assert b[:, 0, 0].tolist() == [0, 500, 1000, 1500, 2000] and b[:, 0, 1].tolist() == [500, 1000, 1500, 2000, 2100]
    assert b[0, :, 2].tolist() == [0, 500, 1000] and b[0, :, 3].tolist() == [500, 1000, 1337]
    # every pixel in exactly one cell
    cover = np.zeros((2100, 1337), np.int32)
    for y0, y1, x0, x1 in b.reshape(-1, 4):
        cover[y0:y1, x0:x1] += 1
    assert (cover == 1).all()


def test_cell_bounds_single_cell_and_tuples():
    from microaligner_amd.shared_modules.registration_qc import cell_bounds
    for cs in (2100, 5000, (3000, 1337)):
        b = cell_bounds((2100, 1337), cs)
        assert b.shape == (1, 1, 4) and b[0, 0].tolist() == [0, 2100, 0, 1337]
    b = cell_bounds((2100, 1337), (1, 1337))
    assert b.shape == (2100, 1, 4) and b[-1, 0].tolist() == [2099, 2100, 0, 1337]
    b = cell_bounds((2100, 1337), (2100, 1))
    assert b.shape == (1, 1337, 4) and b[0, -1].tolist() == [0, 2100, 1336, 1337]
    b = cell_bounds((10, 10), (4, 3))
    assert b.shape == (3, 4, 4) and b[2, 3].tolist() == [8, 10, 9, 10]


def test_arguments_are_validated_before_the_device(monkeypatch):
    from microaligner_amd.shared_modules import registration_qc as Q

    def no_device(*a, **k):
        raise AssertionError("validation must not reach the device")
    monkeypatch.setattr(Q, "get_context", no_device)
    ref = np.zeros((40, 30), np.float32)
    flow = np.zeros((40, 30, 2), np.float32)
    bad = [
        dict(mov_img=np.zeros((40, 31), np.float32)),                  # shape mismatch
        dict(flow=np.zeros((40, 30, 2), np.float64)),                   # flow dtype
        dict(flow=np.zeros((40, 30), np.float32)),                      # flow not (H, W, 2)
        dict(flow=np.zeros((40, 31, 2), np.float32)),                   # flow of another shape
        dict(cell_size=0), dict(cell_size=(10, 0)), dict(cell_size=-3), dict(cell_size=(1, 2, 3)),
        dict(labels="raw"),
        dict(mov_img=np.zeros((40, 30), np.int32)),                     # image dtype
        dict(warped=np.zeros((41, 30), np.float32)),
        dict(ref_img=np.zeros((40, 30, 3), np.float32), mov_img=np.zeros((40, 30, 3), np.float32)),
    ]
    for kw in bad:
        args = dict(ref_img=ref, mov_img=ref, flow=flow)
        args.update(kw)
        with pytest.raises(ValueError):
            Q.assess_registration(**args)
    for f, cs in ((np.zeros((40, 30, 2), np.float64), 10), (np.zeros((40, 30, 3), np.float32), 10),
                  (np.zeros((40, 30), np.float32), 10), (flow, 0)):
        with pytest.raises(ValueError):
            Q.flow_qc(f, cell_size=cs)


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))


def test_qc_header_library_and_bindings_agree():
    from microaligner_amd import _lib, build
    build.build()
    lib = _lib.load()
    names = _declared(QC_HEADER)
    assert names == ["ma_qc_flow_grid", "ma_qc_nmi_grid"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_qc.h but not exported"
    assert sorted(_lib.QC_SIGNATURES) == names, "ctypes prototypes out of sync with microaligner_qc.h"
    assert not set(_lib.QC_SIGNATURES) & set(_lib.SIGNATURES)
    assert '#include "microaligner_hip.h"' in open(QC_HEADER).read()


def test_quality_maps_stay_out_of_the_measured_path_hash(tmp_path, monkeypatch):
    """build.source_hash() names the kernels a profile measured (bench.py quotes PMC traffic only for a matching hash):
    editing qc.hip, its header or the cell grid must leave it unchanged, editing a measured-path source or the gate's
    score, which qc.hip shares with nmi.hip, must change it."""
    import shutil
    from microaligner_amd import build
    assert "qc.hip" in build.SOURCES and QC_HEADER not in [os.path.abspath(h) for h in build.HEADERS]
    out = subprocess.run([sys.executable, "-c", "from microaligner_amd import build; print(build.source_hash())"], cwd=ROOT,
                         capture_output=True, text=True, check=True).stdout.strip()
    assert out == build.source_hash() and re.fullmatch(r"[0-9a-f]{16}", out)
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc)
    # the same headers in the same order: those of csrc from the copy, the public one beside it
    headers = [str((csrc if os.path.samefile(os.path.dirname(h), build.CSRC) else tmp_path) / os.path.basename(h))
               for h in build.HEADERS]
    assert str(csrc / "ma_internal.h") in headers and str(tmp_path / "microaligner_hip.h") in headers
    shutil.copy(os.path.join(ROOT, "include", "microaligner_hip.h"), tmp_path / "microaligner_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADERS", headers)
    assert build.source_hash() == out
    with open(csrc / "qc.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() == out
    with open(csrc / "cell_grid.h", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() == out
    with open(csrc / "nmi_score.h", "a") as f:
        f.write("\n// edited\n")
    scored = build.source_hash()
    assert scored != out
    with open(csrc / "dog.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() not in (out, scored)


# ---- numpy statements ------------------------------------------------------------------------------------------------
def np_det(flow):
    """det J of phi(p) = p + flow(p): numpy.gradient (edge_order=1) of the float64 flow, 0 along an axis of length 1."""
    f = flow.astype(np.float64)
    u, v = f[..., 0], f[..., 1]

    def grad(a, axis):
        return np.gradient(a, axis=axis) if a.shape[axis] > 1 else np.zeros_like(a)
    with np.errstate(invalid="ignore", over="ignore"):
        dudx, dudy, dvdx, dvdy = grad(u, 1), grad(u, 0), grad(v, 1), grad(v, 0)
        return (1 + dudx) * (1 + dvdy) - dudy * dvdx


def np_flow_stats(flow, cell):
    from microaligner_amd.shared_modules.registration_qc import cell_bounds
    H, W = flow.shape[:2]
    b = cell_bounds((H, W), cell)
    gy, gx = b.shape[:2]
    out = {k: np.empty((gy, gx), t) for k, t in (("jac_min", np.float64), ("folded", np.int64), ("invalid", np.int64),
                                                 ("flow_mean", np.float64), ("flow_max", np.float32))}
    for i in range(gy):
        y0, y1 = int(b[i, 0, 0]), int(b[i, 0, 1])
        h0, h1 = max(y0 - 1, 0), min(y1 + 1, H)       # one row of halo: the band's gradients are the image's
        det = np_det(flow[h0:h1])[y0 - h0:y1 - h0]
        f = flow[y0:y1].astype(np.float64)
        fin = np.isfinite(f[..., 0]) & np.isfinite(f[..., 1])
        with np.errstate(invalid="ignore", over="ignore"):
            mag = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1])
        for j in range(gx):
            x0, x1 = int(b[i, j, 2]), int(b[i, j, 3])
            d = det[:, x0:x1]
            d = d[np.isfinite(d)]
            out["jac_min"][i, j] = d.min() if d.size else np.inf
            out["folded"][i, j] = int((d <= 0).sum())
            m = mag[:, x0:x1][fin[:, x0:x1]]
            out["invalid"][i, j] = int((~fin[:, x0:x1]).sum())
            out["flow_mean"][i, j] = m.mean() if m.size else np.nan
            out["flow_max"][i, j] = np.float32(m.max()) if m.size else np.nan
    return out


def assert_flow_stats(q, flow, cell):
    exp = np_flow_stats(flow, cell)
    assert np.array_equal(q.jac_min, exp["jac_min"])
    assert np.array_equal(q.folded, exp["folded"])
    assert np.array_equal(q.invalid, exp["invalid"])
    assert q.flow_max.dtype == np.float32 and np.array_equal(q.flow_max, exp["flow_max"], equal_nan=True)
    fin = np.isfinite(exp["flow_mean"])
    assert np.array_equal(fin, np.isfinite(q.flow_mean))
    np.testing.assert_allclose(q.flow_mean[fin], exp["flow_mean"][fin], rtol=1e-12, atol=0)
    return exp


def crop_nmi(ctx, a, b):
    return ctx.nmi_scores(ctx.asdevice(np.ascontiguousarray(a)), ctx.asdevice(np.ascontiguousarray(b)), 0)[0]


def assert_nmi_cells(ctx, q, ref_l, before_l, after_l, cells=None):
    b = q.cell_bounds
    idx = cells if cells is not None else [(i, j) for i in range(b.shape[0]) for j in range(b.shape[1])]
    for i, j in idx:
        y0, y1, x0, x1 = (int(v) for v in b[i, j])
        r = ref_l[y0:y1, x0:x1]
        assert q.nmi_before[i, j] == crop_nmi(ctx, r, before_l[y0:y1, x0:x1]), (i, j)
        assert q.nmi_after[i, j] == crop_nmi(ctx, r, after_l[y0:y1, x0:x1]), (i, j)


def labels_u8(rng, shape, levels=256):
    return rng.integers(0, levels, size=shape, dtype=np.uint8)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nmi_random_labels_bit_identical_to_gate_on_crops(ctx):
    from microaligner_amd import assess_registration
    rng = np.random.default_rng(11)
    H, W = 2100, 1337
    ref = labels_u8(rng, (H, W))
    mov = ((ref.astype(np.int32) + rng.integers(0, 40, (H, W))) % 256).astype(np.uint8)   # correlated with ref
    wrp = labels_u8(rng, (H, W), 17)
    flow = np.zeros((H, W, 2), np.float32)
    q = assess_registration(ref, mov, flow, cell_size=500, labels="u8", warped=wrp)
    assert q.nmi_before.shape == (5, 3)
    assert_nmi_cells(ctx, q, ref, mov, wrp)
    assert (q.nmi_before > q.nmi_after).all() and not q.improved.any()


@pytest.mark.gpu
def test_nmi_row_and_column_cells(ctx):
    from microaligner_amd import assess_registration
    rng = np.random.default_rng(12)
    H, W = 300, 257
    ref, mov, wrp = labels_u8(rng, (H, W)), labels_u8(rng, (H, W), 8), labels_u8(rng, (H, W), 3)
    flow = np.zeros((H, W, 2), np.float32)
    for cell, shape in (((1, W), (H, 1)), ((H, 1), (1, W)), ((7, 1), (43, W)), ((1, 1), (H, W))):
        q = assess_registration(ref, mov, flow, cell_size=cell, labels="u8", warped=wrp)
        assert q.nmi_before.shape == shape
        cells = None if cell != (1, 1) else [(0, 0), (5, 9), (H - 1, W - 1)]
        assert_nmi_cells(ctx, q, ref, mov, wrp, cells)
        if cell == (1, 1):
            assert (q.nmi_before == 1.0).all() and (q.nmi_after == 1.0).all()   # one pixel: both label sets single-valued
            assert np.isnan(q.ncc_before).all()


@pytest.mark.gpu
def test_nmi_strip_wider_than_a_slice(ctx):
    from microaligner_amd import assess_registration
    rng = np.random.default_rng(13)
    H, W = 3, 70000
    ref, mov, wrp = labels_u8(rng, (H, W)), labels_u8(rng, (H, W), 50), labels_u8(rng, (H, W))
    wrp[:, 1000:] = ref[:, 1000:]
    flow = np.zeros((H, W, 2), np.float32)
    for cell in ((2, 70000), (3, 40000), 70000, (1, 65521)):
        q = assess_registration(ref, mov, flow, cell_size=cell, labels="u8", warped=wrp)
        assert_nmi_cells(ctx, q, ref, mov, wrp)
    # unaligned rows (W odd) as well
    q = assess_registration(ref[:, :69999].copy(), mov[:, :69999].copy(), flow[:, :69999].copy(), cell_size=(2, 66001),
                            labels="u8", warped=wrp[:, :69999].copy())
    assert_nmi_cells(ctx, q, ref[:, :69999], mov[:, :69999], wrp[:, :69999])


@pytest.mark.gpu
def test_nmi_constant_cells_and_sklearn(ctx):
    from sklearn.metrics import normalized_mutual_info_score
    from microaligner_amd import assess_registration
    rng = np.random.default_rng(14)
    H, W = 400, 333
    ref = labels_u8(rng, (H, W), 5)
    mov = labels_u8(rng, (H, W), 200)
    wrp = ref.copy()
    ref[:100, :100] = 7
    mov[:100, :100] = 200
    wrp[:100, :100] = 3
    mov[100:200, :100] = 9          # mov constant, ref not
    flow = np.zeros((H, W, 2), np.float32)
    q = assess_registration(ref, mov, flow, cell_size=100, labels="u8", warped=wrp)
    assert_nmi_cells(ctx, q, ref, mov, wrp)
    assert q.nmi_before[0, 0] == 1.0 and q.nmi_after[0, 0] == 1.0
    assert abs(q.nmi_before[1, 0]) < 1e-12          # mov's labels constant, ref's not: no mutual information
    assert np.isnan(q.ncc_before[0, 0]) and np.isnan(q.ncc_after[0, 0]) and np.isnan(q.ncc_before[1, 0])
    for i, j in ((0, 0), (1, 0), (2, 1), (3, 3), (1, 2)):
        y0, y1, x0, x1 = (int(v) for v in q.cell_bounds[i, j])
        for got, other in ((q.nmi_before, mov), (q.nmi_after, wrp)):
            exp = normalized_mutual_info_score(ref[y0:y1, x0:x1].ravel(), other[y0:y1, x0:x1].ravel())
            assert abs(got[i, j] - exp) <= 1e-12, (i, j, got[i, j], exp)


@pytest.mark.gpu
def test_ncc_matches_corrcoef(ctx):
    from microaligner_amd import assess_registration
    rng = np.random.default_rng(15)
    H, W = 611, 517
    ref = labels_u8(rng, (H, W))
    mov = np.clip(ref.astype(np.int32) + rng.integers(-60, 60, (H, W)), 0, 255).astype(np.uint8)
    wrp = (255 - ref).astype(np.uint8)
    wrp[:128, :128] = 77
    flow = np.zeros((H, W, 2), np.float32)
    q = assess_registration(ref, mov, flow, cell_size=128, labels="u8", warped=wrp)
    for i in range(q.cell_bounds.shape[0]):
        for j in range(q.cell_bounds.shape[1]):
            y0, y1, x0, x1 = (int(v) for v in q.cell_bounds[i, j])
            a = ref[y0:y1, x0:x1].ravel().astype(np.float64)
            for got, other in ((q.ncc_before, mov), (q.ncc_after, wrp)):
                b = other[y0:y1, x0:x1].ravel().astype(np.float64)
                if b.min() == b.max():
                    assert np.isnan(got[i, j])
                else:
                    assert abs(got[i, j] - np.corrcoef(a, b)[0, 1]) <= 1e-12, (i, j)
    assert q.ncc_after[1, 1] == -1.0 and q.ncc_before[1, 1] > 0.7


@pytest.mark.gpu
def test_nmi_dog_labels_bit_identical_to_gate_on_crops(ctx):
    from microaligner_amd import Warper, assess_registration, synthetic
    ref, mov = synthetic.make_pair(2100, 1337, 3)
    rng = np.random.default_rng(16)
    flow = (rng.standard_normal((2100, 1337, 2)) * 1.5).astype(np.float32)
    q = assess_registration(ref, mov, flow, cell_size=500, tile_size=600, overlap=50)
    w = Warper()
    w.tile_size, w.overlap, w.image, w.flow = 600, 50, mov, flow
    wrp = w.warp()
    lab = [ctx.dog_u8(ctx.asdevice(x)).numpy() for x in (ref, mov, wrp)]
    assert_nmi_cells(ctx, q, *lab)


@pytest.mark.gpu
def test_flow_statistics_against_numpy(ctx):
    from microaligner_amd import flow_qc
    H, W = 701, 1029
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cases = {}
    cases["zero"] = np.zeros((H, W, 2), np.float32)
    t = np.empty((H, W, 2), np.float32)
    t[..., 0], t[..., 1] = 3.5, -2.25
    cases["translation"] = t
    s, th = 1.3, 0.4                      # phi(p) = A p, det A = s^2
    A = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    sr = np.empty((H, W, 2), np.float32)
    sr[..., 0] = (A[0, 0] - 1) * xx + A[0, 1] * yy
    sr[..., 1] = A[1, 0] * xx + (A[1, 1] - 1) * yy
    cases["scale_rotation"] = sr
    fold = np.zeros((H, W, 2), np.float32)
    fold[200:260, :, 0] = -2.0 * xx[200:260]   # du/dx = -2 on 60 full rows, dv/dx = 0: det = -1 there, 1 elsewhere
    cases["fold"] = fold
    rng = np.random.default_rng(17)
    nanf = (rng.standard_normal((H, W, 2)) * 0.4).astype(np.float32)
    nanf[100:130, 40:90, 0] = np.nan
    nanf[500, 1000, 1] = np.inf
    nanf[0, 0, 0] = -np.inf
    nanf[690:701, 1020:1029] = np.nan
    nanf[300, 300] = np.nan
    cases["nan_patches"] = nanf
    for name, f in cases.items():
        for cell in (256, (100, 1029), (701, 37), 5000):
            q = flow_qc(f, cell_size=cell)
            exp = assert_flow_stats(q, f, cell)
            if name in ("zero", "translation"):
                assert (q.jac_min == 1.0).all() and (q.folded == 0).all() and (q.invalid == 0).all()
            if name == "scale_rotation":
                assert abs(q.jac_min.min() - s * s) < 1e-4 and q.folded.sum() == 0
            if name == "fold":
                assert q.folded.sum() == 60 * W and q.jac_min.min() == -1.0
            if name == "nan_patches":
                assert q.invalid.sum() == 30 * 50 + 1 + 1 + 11 * 9 + 1
                assert exp["folded"].sum() == q.folded.sum()
    s1 = flow_qc(cases["nan_patches"][:1], cell_size=64)      # axes of length 1: derivative 0
    assert_flow_stats(s1, cases["nan_patches"][:1], 64)
    s2 = flow_qc(np.ascontiguousarray(cases["nan_patches"][:, :1]), cell_size=64)
    assert_flow_stats(s2, np.ascontiguousarray(cases["nan_patches"][:, :1]), 64)


@pytest.mark.gpu
def test_agrees_with_the_gate_of_register(ctx):
    from microaligner_amd import OptFlowRegistrator, assess_registration, synthetic
    ref, mov = synthetic.make_pair(2000, 1000, 5)
    reg = OptFlowRegistrator()
    reg.verbose = False
    reg.num_pyr_lvl, reg.use_full_res_img, reg.tile_size = 0, True, 1000
    reg.ref_img, reg.mov_img = ref, mov
    flow = reg.register()
    rep = reg.level_reports[0]
    assert rep.accepted
    q = assess_registration(ref, mov, flow, cell_size=1000, tile_size=1000, overlap=100)
    assert q.nmi_after.shape == (2, 1)
    assert np.mean(q.nmi_after) == rep.mi_after
    assert np.mean(q.nmi_before) == rep.mi_before
    s = q.summary()
    assert s["cells"] == 2 and s["cells_improved"] == int(q.improved.sum())


@pytest.mark.gpu
def test_results_do_not_depend_on_inputs_batching_or_repetition(ctx):
    from microaligner_amd import _lib as L
    from microaligner_amd import assess_registration, flow_qc, synthetic
    ref, mov = synthetic.make_pair(1100, 1337, 7, dtype=np.uint16)
    rng = np.random.default_rng(18)
    flow = (rng.standard_normal((1100, 1337, 2)) * 2).astype(np.float32)
    flow[5:9, 700:720] = np.nan

    def fields(q):
        return [q.cell_bounds, q.nmi_before, q.nmi_after, q.ncc_before, q.ncc_after, q.flow_mean, q.flow_max, q.jac_min,
                q.folded, q.invalid]

    def same(a, b):
        for x, y in zip(fields(a), fields(b)):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)

    for labels in ("dog", "u8"):
        base = assess_registration(ref, mov, flow, cell_size=(300, 250), labels=labels)
        same(base, assess_registration(ref, mov, flow, cell_size=(300, 250), labels=labels))
        d = [ctx.asdevice(x) for x in (ref, mov, flow)]
        same(base, assess_registration(*d, cell_size=(300, 250), labels=labels))
        wrp = ctx.warp(d[1], d[2], 1000, 100)
        same(base, assess_registration(ref, mov, flow, cell_size=(300, 250), labels=labels, warped=wrp))
        same(base, assess_registration(ref, mov, flow, cell_size=(300, 250), labels=labels, warped=wrp.numpy()))
        prev = ctx.get_option(L.MA_OPT_WORKSPACE_LIMIT)
        try:
            ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, 1 << 20)     # 2 cells per batch of the NMI pass
            small = assess_registration(ref, mov, flow, cell_size=(300, 250), labels=labels)
            tiny_cells = flow_qc(flow, cell_size=(3, 2))         # > 65535 cells: several batches of the flow pass
        finally:
            ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, prev)
        same(base, small)
        big = flow_qc(flow, cell_size=(3, 2))
        for k in ("flow_mean", "flow_max", "jac_min", "folded", "invalid"):
            assert np.array_equal(getattr(tiny_cells, k), getattr(big, k), equal_nan=True)
    assert_flow_stats(big, flow, (3, 2))


@pytest.mark.gpu
def test_nmi_grid_one_image_batches(ctx):
    """ma_qc_nmi_grid without b1 (assess_registration always passes two images): the batch's results lie at pin[i] and
    pin[nb + i].  Under a 1 MiB workspace limit a cell and image take 262 576 B, so the one-image call runs in batches of
    3 cells and the two-image call in batches of 1."""
    from microaligner_amd import _lib as L
    rng = np.random.default_rng(20)
    H, W, cell = 100, 90, (32, 40)
    ref, l0, l1 = labels_u8(rng, (H, W)), labels_u8(rng, (H, W)), labels_u8(rng, (H, W))
    d_ref, b0, b1 = (ctx.asdevice(x) for x in (ref, l0, l1))
    full = ctx.qc_nmi_grid(d_ref, b0, None, *cell)
    prev = ctx.get_option(L.MA_OPT_WORKSPACE_LIMIT)
    try:
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, 1 << 20)
        one = ctx.qc_nmi_grid(d_ref, b0, None, *cell)
        two = ctx.qc_nmi_grid(d_ref, b0, b1, *cell)
    finally:
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, prev)
    nmi0, nmi1, ncc0, ncc1 = one
    assert nmi1 is None and ncc1 is None and full[1] is None and full[3] is None
    assert nmi0.shape == (4, 3) and ncc0.shape == (4, 3)
    for got in (two, full):
        assert np.array_equal(nmi0, got[0]) and np.array_equal(ncc0, got[2])
    assert np.isfinite(ncc0).all()
    for i in range(4):
        for j in range(3):
            y0, x0 = 32 * i, 40 * j
            assert nmi0[i, j] == crop_nmi(ctx, ref[y0:y0 + 32, x0:x0 + 40], l0[y0:y0 + 32, x0:x0 + 40]), (i, j)


@pytest.mark.gpu
def test_large_grid_8192(ctx):
    from microaligner_amd import assess_registration, synthetic
    H = W = 8192
    ref, mov = synthetic.make_pair(H, W, 9)
    rng = np.random.default_rng(19)
    yy = np.linspace(0, 6 * np.pi, H, dtype=np.float32)[:, None]
    xx = np.linspace(0, 4 * np.pi, W, dtype=np.float32)[None, :]
    flow = np.empty((H, W, 2), np.float32)
    flow[..., 0] = 2.0 * np.sin(yy) + 0.01 * rng.standard_normal((H, W), dtype=np.float32)
    flow[..., 1] = 1.5 * np.cos(xx) + 0.01 * rng.standard_normal((H, W), dtype=np.float32)
    flow[4000:4003, 100:200] = np.nan
    flow[7000:7040, 5000:5100, 0] *= -400.0   # folds
    q = assess_registration(ref, mov, flow, cell_size=1000)
    assert q.nmi_before.shape == (9, 9)
    d = [ctx.asdevice(x) for x in (ref, mov)]
    wrp = ctx.warp(d[1], ctx.asdevice(flow), 1000, 100)
    lab = [ctx.dog_u8(x).numpy() for x in (d[0], d[1], wrp)]
    assert_nmi_cells(ctx, q, *lab, cells=[(0, 0), (3, 5), (4, 0), (7, 7), (8, 2), (2, 8), (8, 8)])
    assert_flow_stats(q, flow, 1000)
    assert q.folded.sum() > 0 and q.invalid.sum() == 300
