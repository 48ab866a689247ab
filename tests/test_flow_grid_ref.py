"""Grid flows on the CPU (no GPU): the numpy statement of include/microaligner_flowgrid.h (tests/_flow_grid_ref.py) held
to its stated properties, to an independent float64 expansion within a derived rounding bound, to the analytic bound of
bilinear interpolation, and its point sampler to the float64 sampler of microaligner_flowinvert.h on the expanded flow;
the stride chooser, FlowGrid's checks and file format, the SaveFlowGridStride schema and the plumbing of the new header."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_grid_ref as G  # noqa: E402
import _flow_invert_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402
from microaligner_amd import FlowGrid, _lib, build  # noqa: E402
from microaligner_amd.device import affine_flow_params, affine_grid_params, grid_nodes, transform_points_params  # noqa: E402
from microaligner_amd.optflow_reg import flow_grid as FG  # noqa: E402
from microaligner_amd.pipeline import RegParam  # noqa: E402

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowgrid.h")
SIZES = [(1, 1), (1, 7), (5, 1), (17, 18), (33, 65), (9, 10)]
STRIDES = [1, 2, 3, 7, 16, 300]


def seeded_flow(shape, seed=0):
    return np.random.default_rng(seed).uniform(-20, 20, shape + (2,)).astype(F32)


# ---- the axis -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 7, 16])
def test_axis_nodes_positions_and_the_last_short_interval(s):
    for n in sorted({1, 2, s, s + 1, s + 2, 2 * s + 1}):
        g, P = G.grid_nodes(n, s), G.node_positions(n, s)
        assert g == grid_nodes(n, s) == len(P)
        if n == 1:
            assert g == 1 and P.tolist() == [0]
            continue
        assert g == int(np.ceil((n - 1) / s)) + 1
        assert P[0] == 0 and P[-1] == n - 1 and np.all(np.diff(P) >= 1) and np.all(np.diff(P[:-1]) == s)
        assert 1 <= P[-1] - P[-2] <= s
        i0, i1, t = G.axis(n, s)
        x = np.arange(n)
        assert np.all(P[i0] <= x) and np.all(x <= P[i1]) and np.all(i1 == i0 + 1)
        assert t.dtype == F32 and t.min() >= 0 and t.max() <= 1
        assert np.all(t[P[:-1]] == 0) and t[n - 1] == 1     # a node is the start of its cell, the last one the end of its


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (17, 18)])
def test_a_stride_above_the_image_is_one_cell_or_one_node(shape):
    H, W = shape
    nodes = G.sample_ref(seeded_flow(shape), 300)
    assert nodes.shape == (1 if H == 1 else 2, 1 if W == 1 else 2, 2)
    assert np.array_equal(nodes, G.sample_ref(seeded_flow(shape), max(H, W)))
    assert np.array_equal(G.expand_ref(nodes, shape, 300), G.expand_ref(nodes, shape, max(H, W)))


# ---- expand: the stated properties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", STRIDES)
@pytest.mark.parametrize("shape", SIZES)
def test_expand_gives_finite_nodes_back_and_stride_one_is_the_flow(shape, s):
    f = seeded_flow(shape, 1)
    nodes = G.sample_ref(f, s)
    e = G.expand_ref(nodes, shape, s)
    Py, Px = G.node_positions(shape[0], s), G.node_positions(shape[1], s)
    assert np.array_equal(e[Py][:, Px], nodes)
    if s == 1:
        assert np.array_equal(e.view(np.uint32), f.view(np.uint32))     # no zeros of either sign in a uniform draw


@pytest.mark.parametrize("s", [2, 3, 7])
def test_a_non_finite_node_reaches_exactly_the_cells_it_is_a_corner_of(s):
    shape = (17, 18)
    nodes = G.sample_ref(seeded_flow(shape, 2), s)
    Py, Px = G.node_positions(shape[0], s), G.node_positions(shape[1], s)
    for (j, i), v in itertools.product([(0, 0), (1, 2), (len(Py) - 1, len(Px) - 1), (2, len(Px) - 1)], [np.nan, np.inf]):
        bad = nodes.copy()
        bad[j, i, 0] = v
        e = G.expand_ref(bad, shape, s)
        # a pixel's cell is min(x // s, g - 2); node k is a corner of the cells k - 1 and k
        cy, cx = np.minimum(np.arange(shape[0]) // s, len(Py) - 2), np.minimum(np.arange(shape[1]) // s, len(Px) - 2)
        exp = (((cy == j) | (cy == j - 1))[:, None]) & (((cx == i) | (cx == i - 1))[None, :])
        hit = ~np.isfinite(e[..., 0])
        assert np.array_equal(hit, exp), (j, i, v)
        assert np.isfinite(e[..., 1]).all()


# ---- expand: against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", STRIDES)
@pytest.mark.parametrize("shape", SIZES + [(301, 417)])
def test_float32_expand_is_within_the_derived_rounding_of_float64(shape, s):
    """bound: _flow_grid_ref.EXPAND_ROUNDING (derived there) times max |node|"""
    nodes = G.sample_ref(seeded_flow(shape, 3), s)
    got = np.abs(G.expand_ref(nodes, shape, s).astype(F64) - G.expand_f64(nodes, shape, s)).max()
    bound = G.EXPAND_ROUNDING * float(np.abs(nodes).max())
    print(f"{shape} s={s}: {got:.3g} <= {bound:.3g} ({got / bound:.2f})")
    assert got <= bound


@pytest.mark.parametrize("apq", [(3, 180, 240), (25, 400, 300), (1, 64, 90)])
@pytest.mark.parametrize("s", [2, 4, 8, 16, 32])
def test_expand_of_a_sampled_sine_is_within_the_bilinear_bound(s, apq):
    """f = A sin(2 pi x / P) cos(2 pi y / Q), the second component with the axes swapped: bilinear interpolation on
    cells of at most s x s is within s^2 / 8 (max |fxx| + max |fyy|) = s^2 / 8 A (2 pi)^2 (1 / P^2 + 1 / Q^2); on top the
    float32 rounding of the nodes (U A, kept by a convex combination) and of the expansion."""
    A, P, Q = apq
    H, W = 301, 417
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    f = np.stack([A * np.sin(2 * np.pi * x / P) * np.cos(2 * np.pi * y / Q),
                  A * np.sin(2 * np.pi * y / P) * np.cos(2 * np.pi * x / Q)], -1)
    e = G.expand_ref(G.sample_ref(f.astype(F32), s), (H, W), s)
    got = np.abs(e.astype(F64) - f).max()
    bound = s * s / 8 * A * (2 * np.pi) ** 2 * (1 / P ** 2 + 1 / Q ** 2) + (G.U + G.EXPAND_ROUNDING) * A
    print(f"s={s} {apq}: {got:.6g} <= {bound:.6g}")
    assert got <= bound


# ---- loss maps ------------------------------------------------------------------------------------------------------------
def test_loss_maps_count_what_the_definition_says():
    shape, s = (33, 65), 7
    f = G.smooth_flow(shape, 4)
    nodes = G.sample_ref(f, s)
    e = G.expand_ref(nodes, shape, s)
    f2 = f.copy()
    f2[3, 4, 0] = np.nan            # invalid
    f2[20, 50] = np.inf             # E - Inf = -Inf: valid, error Inf
    f2[32, 64, 1] = e[32, 64, 1] + F32(0.5)      # the ragged corner cell of one pixel
    max_err, above, invalid = G.error_maps_ref(f2, nodes, s, (16, 16), 0.25)
    assert max_err.shape == (3, 5) and invalid.sum() == 1 and invalid[0, 0] == 1
    assert max_err[1, 3] == np.inf and above[1, 3] == 1
    assert abs(max_err[2, 4] - 0.5) < 1e-5 and above[2, 4] == 1 and above.sum() == 2
    whole = G.error_maps_ref(f, nodes, s, (1000, 1000), 0.0)
    assert whole[0].shape == (1, 1) and whole[2][0, 0] == 0
    assert whole[0][0, 0] == np.abs(e - f).max() and whole[1][0, 0] == int((np.abs(e - f).max(-1) > 0).sum())
    # a cell without a valid pixel
    f3 = np.full(shape + (2,), np.nan, F32)
    m3 = G.error_maps_ref(f3, nodes, s, (16, 16), 0.25)
    assert np.isnan(m3[0]).all() and m3[1].sum() == 0 and m3[2].sum() == 33 * 65


# ---- the point sampler -------------------------------------------------------------------------------------------------------
def seeded_points(shape, s, n=4000, seed=5):
    H, W = shape
    r = np.random.default_rng(seed)
    pts = np.stack([r.uniform(-5, W + 4, n), r.uniform(-5, H + 4, n)], -1)
    Px, Py = G.node_positions(W, s), G.node_positions(H, s)
    border = np.array([(px, py) for px in Px[:4].tolist() + [Px[-1]] for py in Py[:3].tolist() + [Py[-1]]], F64)
    mixed = np.stack([r.choice(Px, 50).astype(F64), r.uniform(0, H - 1, 50)], -1)      # on cell borders along x only
    edge = np.array([(0, 0), (W - 1, H - 1), (W - 1, 0.5), (0.5, H - 1), (-3, 2), (W + 2, H + 2)], F64)
    special = np.array([(np.nan, 1), (1, np.nan), (np.inf, 2), (3, -np.inf)], F64)
    return np.concatenate([pts, border, mixed, edge, special])


@pytest.mark.parametrize("s", [1, 3, 8, 300])
@pytest.mark.parametrize("shape", [(33, 65), (9, 10), (1, 7), (5, 1)])
def test_point_sampler_equals_the_float64_sampler_on_the_expanded_flow(shape, s):
    """G64 on the nodes against S64 (tests/_flow_invert_ref.py) on expand(grid): in real arithmetic the same function;
    S64 takes its four taps from the float32 expansion, each within EXPAND_ROUNDING M of the exact one, and combines them
    convexly; 1e-12 M for the float64 roundings of both."""
    f = G.smooth_flow(shape, 6)
    nodes = G.sample_ref(f, s)
    e = G.expand_ref(nodes, shape, s)
    pts = seeded_points(shape, s)
    M = float(np.abs(nodes).max())
    bound = (G.EXPAND_ROUNDING + 1e-12) * M
    got, conv, inside = G.to_moving_grid_ref(pts, nodes, shape, s)
    exp, econv, einside = R.to_moving_ref(pts, e)
    assert np.array_equal(conv, econv) and np.array_equal(inside, einside)
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.isnan(got[-4:]).all()
    err = np.nanmax(np.abs(got - exp))
    print(f"{shape} s={s}: {err:.3g} <= {bound:.3g}")
    assert err <= bound
    # through a matrix and a padding: the difference is multiplied by at most the matrix' largest absolute row sum
    tmat = np.array([[0.98, -0.05, 1.5], [0.05, 0.98, -2.0]])
    _, m, left, top = affine_flow_params((max(shape[0] - 2, 1), max(shape[1] - 3, 1)), F32, shape + (2,), F32, tmat)
    got = G.to_moving_grid_ref(pts, nodes, shape, s, m, (left, top))[0]
    exp = R.to_moving_ref(pts, e, m, (left, top))[0]
    norm = np.abs(m.reshape(2, 3)[:, :2]).sum(1).max()
    assert np.nanmax(np.abs(got - exp)) <= norm * bound + 1e-12 * max(shape)


@pytest.mark.parametrize("s", [3, 8])
def test_point_round_trip_on_a_grid_within_l_tol(s):
    """the bound of test_flow_invert_ref.py: to_reference stops within tol of its fixed point, so the round trip is off
    by at most L tol (+ 1e-9 for the float64 roundings), L the Lipschitz constant of the sampled function -- here the
    bilinear function on the nodes, whose slopes are the adjacent differences of its expansion."""
    shape, tol = (120, 150), 1e-4
    nodes = G.sample_ref(G.smooth_flow(shape, 7, amp=4.0), s)
    L = R.lipschitz(G.expand_f64(nodes, shape, s).astype(F32)) + 1e-6
    assert L < 1
    r = np.random.default_rng(8)
    q = np.stack([r.uniform(10, shape[1] - 11, 3000), r.uniform(10, shape[0] - 11, 3000)], -1)
    p, conv, inside = G.to_reference_grid_ref(q, nodes, shape, s, max_iter=60, tol=tol)
    assert conv.all() and inside.all()
    back = G.to_moving_grid_ref(p, nodes, shape, s)[0]
    err = float(np.abs(back - q).max())
    print(f"s={s}: round trip {err:.3g} px, bound {L * tol + 1e-9:.3g}")
    assert err <= L * tol + 1e-9


# ---- the stride chooser -------------------------------------------------------------------------------------------------------
def test_stride_choice_on_the_statements_maps():
    """choose_stride on error_maps_ref: the largest stride within tol; an invalid pixel disqualifies every stride but 1"""
    shape = (130, 140)
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(F64)
    f = np.stack([5 * np.sin(2 * np.pi * x / 200), 5 * np.cos(2 * np.pi * y / 200)], -1).astype(F32)

    def maps_of(flow):
        return lambda s: G.error_maps_ref(flow, G.sample_ref(flow, s), s, (50, 50), tol)

    for tol in (1 / 32, 1 / 256, 1e-7, 10.0):
        errs = {s: FG.global_max_err(maps_of(f)(s)[0]) for s in FG.STRIDES}
        exp = next((s for s in FG.STRIDES if errs[s] <= tol), 1)
        got, maps = FG.choose_stride(maps_of(f), tol)
        print(tol, got, errs)
        assert got == exp and FG.global_max_err(maps[0]) == errs[got]
    # s^2 / 8 * 5 (2 pi / 200)^2 is 0.0099 px at s = 4: within 1/32, so the choice is at least 4; no error exceeds 2 A = 10
    tol = 1 / 32
    assert FG.choose_stride(maps_of(f), tol)[0] >= 4
    tol = 10.0
    assert FG.choose_stride(maps_of(f), tol)[0] == 64
    bad = f.copy()
    bad[7, 9, 0] = np.nan
    tol = 10.0
    s, maps = FG.choose_stride(maps_of(bad), tol)
    assert s == 1 and maps[2].sum() == 4      # at stride 1 a NaN pixel is a corner of four one-pixel cells (NaN * 0 = NaN)
    assert not FG.qualifies(np.array([[np.nan]], F32), np.array([[0]]), 1.0)      # no valid pixel qualifies nothing


# ---- FlowGrid: checks and the file format --------------------------------------------------------------------------------------
def test_flow_grid_refuses_what_does_not_fit():
    nodes = np.zeros((3, 4, 2), F32)      # g(17, 8) = 3, g(18, 7) would be 4
    g = FlowGrid(np.zeros((3, 4, 2), F32), 8, (17, 25))
    assert g.shape == (17, 25) and g.stride == 8 and g.nbytes == 3 * 4 * 2 * 4 and len(g) == 3
    for bad in (dict(nodes=nodes.astype(F64)), dict(nodes=nodes[:2]), dict(nodes=nodes[..., :1]), dict(nodes=nodes.tolist()),
                dict(stride=0), dict(stride=-1), dict(stride=2.0), dict(stride=True), dict(stride=1 << 31), dict(stride=7),
                dict(shape=(17,)), dict(shape=(17, 26)), dict(shape=(0, 25)), dict(shape=(17.0, 25)), dict(shape=None)):
        args = dict(nodes=nodes, stride=8, shape=(17, 25))
        args.update(bad)
        with pytest.raises(ValueError):
            FlowGrid(**args)
    with pytest.raises(ValueError):
        affine_grid_params((17, 24), np.uint8, g, None)               # without tmat the image has the grid's shape
    with pytest.raises(ValueError):
        affine_grid_params((17, 25), np.int32, g, None)
    with pytest.raises(ValueError):
        affine_grid_params((17, 25), np.uint8, np.zeros((17, 25, 2), F32), None)
    assert affine_grid_params((17, 25), np.uint8, g, None, "nearest")[1:] == (pytest.approx([1, 0, 0, 0, 1, 0]), 0, 0)
    assert affine_grid_params((15, 21), np.uint8, g, [[1, 0, 0], [0, 1, 0]])[2:] == (2, 1)
    pts = np.zeros((3, 2))
    assert transform_points_params(pts, g, "to_moving", None, None, 50, 1e-4)[1] == _lib.MA_POINTS_TO_MOVING
    with pytest.raises(ValueError):
        transform_points_params(pts.astype(F32), g, "to_moving", None, None, 50, 1e-4)


def test_flow_grid_file_round_trip_and_version(tmp_path):
    nodes = seeded_flow((3, 4), 9)
    nodes[1, 2] = (np.nan, -0.0)
    g = FlowGrid(nodes, 8, (17, 25))
    path = tmp_path / "grid.npz"
    g.save(path)
    back = FlowGrid.load(path)
    assert back.stride == 8 and back.shape == (17, 25) and isinstance(back.nodes, np.ndarray)
    assert np.array_equal(back.nodes.view(np.uint32), nodes.view(np.uint32))
    with np.load(path) as z:
        assert sorted(z.files) == ["format_version", "nodes", "shape", "stride"] and int(z["format_version"]) == 1
        fields = {k: z[k] for k in z.files}
    fields["format_version"] = np.int64(2)
    np.savez(tmp_path / "v2.npz", **fields)
    with pytest.raises(ValueError, match="format version 2"):
        FlowGrid.load(tmp_path / "v2.npz")
    del fields["stride"]
    np.savez(tmp_path / "short.npz", **fields)
    with pytest.raises(ValueError, match="not a FlowGrid file"):
        FlowGrid.load(tmp_path / "short.npz")


# ---- the CLI key -------------------------------------------------------------------------------------------------------------
def test_save_flow_grid_stride_schema():
    base = dict(NumberPyramidLevels=3, NumberIterationsPerLevel=3, TileSize=1000, Overlap=100, NumberOfWorkers=0,
                UseFullResImage=False, UseDOG=True)
    assert RegParam(dict(base), optflow=True).SaveFlowGridStride is None
    assert RegParam(dict(base, SaveFlowGridStride=8), optflow=True).SaveFlowGridStride == 8
    assert RegParam(dict(base, SaveFlowGridStride=1), optflow=True).SaveFlowGridStride == 1
    for bad in ("8", 8.0, None, True, [8]):
        with pytest.raises(TypeError):
            RegParam(dict(base, SaveFlowGridStride=bad), optflow=True)
    for bad in (0, -4):
        with pytest.raises(ValueError):
            RegParam(dict(base, SaveFlowGridStride=bad), optflow=True)
    with pytest.raises(ValueError, match="OptFlowReg only"):
        RegParam(dict(base, SaveFlowGridStride=8), optflow=False)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_build_recipe_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.FLOWGRID_SIGNATURES) and len(declared) == 6
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    assert "flow_grid.hip" in build.SOURCES
    assert any(os.path.samefile(h, HEADER) for h in build.SOURCE_HEADERS["flow_grid.hip"])
    for src in ("warp_compose.hip", "flow_invert.hip"):       # their kernels take the flow from a grid too
        assert any(os.path.samefile(h, HEADER) for h in build.GRID_FLOW_USERS[src])
    assert not any(os.path.samefile(h, HEADER) for h in build.HEADERS)


def test_the_measured_path_is_untouched():
    """build.source_hash() is the value of the commit before grid flows (README, "Grid flows")"""
    assert build.source_hash() == HASH


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    assert lib.ma_flow_grid_sample(None, None, 4, 4, 2, None) == _lib.MA_EINVAL
    assert lib.ma_flow_grid_expand(None, None, 4, 4, 2, None) == _lib.MA_EINVAL
    assert lib.ma_flow_grid_error(None, None, None, 4, 4, 2, 2, 2, 0.1, None, None, None) == _lib.MA_EINVAL
    assert lib.ma_warp_affine_grid(None, None, 0, 4, 4, 0, 0, None, 4, 4, 2, None, None, 1) == _lib.MA_EINVAL
    assert lib.ma_transform_points_grid(None, None, 0, None, 4, 4, 2, None, None, 0, 0, 0, 5, 1e-4, None, None,
                                        None) == _lib.MA_EINVAL
