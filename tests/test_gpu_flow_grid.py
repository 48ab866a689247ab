"""-m gpu: grid flows on the device.  ma_flow_grid_sample / _expand / _error and ma_transform_points_grid against the numpy
statement of include/microaligner_flowgrid.h (tests/_flow_grid_ref.py) bit for bit, at the smallest shapes that reach the
block edges of the 64 x 32 tile; the Python entries; the CLI key."""
import os
import re
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_grid_ref as G  # noqa: E402
from microaligner_amd import (FlowGrid, FlowGridError, OptFlowRegistrator, Warper, _lib, compose_flows, compress_flow,  # noqa: E402
                              flow_grid_error, flow_qc, invert_flow, synthetic, transform_points)
from microaligner_amd import pipeline as P  # noqa: E402
from microaligner_amd.device import DeviceArray, affine_flow_params  # noqa: E402
from microaligner_amd.optflow_reg import flow_grid as FG  # noqa: E402
from microaligner_amd.shared_modules.utils import max_project_and_normalize  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64

# block edges of the 64-column tile and of its 32 rows; W = k s + 1 and k s + 2 for the strides below
SHAPES = [(1, 1), (1, 7), (5, 1), (17, 18), (63, 64), (65, 130), (33, 257)]
STRIDES = [1, 2, 3, 7, 16, 64, 300]
CELLS = [(16, 16), (5, 40), (1000, 1000)]


def same_bits(got, exp):
    """equal as bit patterns, any NaN payload standing for NaN"""
    assert got.dtype == exp.dtype and got.shape == exp.shape
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(got.view(u)[~gn], exp.view(u)[~en])


def test_shapes_cover_the_last_short_and_full_intervals():
    assert any((W - 1) % s == 0 and W > s for _, W in SHAPES for s in STRIDES if s > 1)        # W = k s + 1
    assert any((W - 2) % s == 0 and W > s + 1 for _, W in SHAPES for s in STRIDES if s > 1)    # W = k s + 2


@pytest.mark.parametrize("poisoned", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_expand_and_loss_equal_the_statement(ctx, shape, poisoned):
    f = G.smooth_flow(shape, 11)
    if poisoned:
        f = G.poison(f, 12)
    d_f = ctx.asdevice(f)
    for s in STRIDES:
        exp_nodes = G.sample_ref(f, s)
        grid = ctx.flow_grid_sample(d_f, s)
        assert grid.stride == s and grid.shape == shape and isinstance(grid.nodes, DeviceArray)
        assert same_bits(grid.nodes.numpy(), exp_nodes), s
        # the loss of the sampled grid, and of nodes that carry non-finite values of their own
        nodes = G.poison(exp_nodes, 13 + s, 2) if poisoned else exp_nodes
        grid = FlowGrid(nodes, s, shape)
        exp = G.expand_ref(nodes, shape, s)
        assert same_bits(ctx.flow_grid_expand(grid).numpy(), exp), s
        for cell in CELLS:
            em, ea, ei = G.error_maps_ref(f, nodes, s, cell, 1 / 32)
            gm, ga, gi = ctx.flow_grid_error(d_f, grid, cell[0], cell[1], 1 / 32)
            assert same_bits(gm, em) and np.array_equal(ga, ea) and np.array_equal(gi, ei), (s, cell)
            if np.isnan(f).any():
                assert ei.sum() > 0
        if not poisoned and s == 1:
            assert em.max() == 0 and ea.sum() == 0 and ei.sum() == 0


def test_loss_counts_above_tol_and_batches_cells(ctx):
    """a tolerance that splits the pixels; 1 x 1 cells (every pixel its own cell), ragged cells, one cell"""
    shape, s = (40, 70), 7
    f = G.smooth_flow(shape, 14, amp=9.0)
    nodes = G.sample_ref(f, s)
    grid = FlowGrid(nodes, s, shape)
    whole = G.error_maps_ref(f, nodes, s, shape, 0.0)[0][0, 0]
    tol = float(whole) / 3
    for cell in [(1, 1), (7, 9), (40, 70)]:
        em, ea, ei = G.error_maps_ref(f, nodes, s, cell, tol)
        gm, ga, gi = ctx.flow_grid_error(ctx.asdevice(f), grid, cell[0], cell[1], tol)
        assert same_bits(gm, em) and np.array_equal(ga, ea) and np.array_equal(gi, ei), cell
        assert 0 < ea.sum() < shape[0] * shape[1]


# ---- points -------------------------------------------------------------------------------------------------------------
def grid_points(shape, s, seed):
    H, W = shape
    r = np.random.default_rng(seed)
    Px, Py = G.node_positions(W, s), G.node_positions(H, s)
    return np.concatenate([
        np.stack([r.uniform(-4, W + 3, 3000), r.uniform(-4, H + 3, 3000)], -1),
        np.array([(px, py) for px in Px[:5].tolist() + [Px[-1]] for py in Py[:4].tolist() + [Py[-1]]], F64),
        np.stack([r.choice(Px, 40).astype(F64), r.uniform(0, H - 1, 40)], -1),
        np.array([(0, 0), (W - 1, H - 1), (W - 1, 0.25), (0.25, H - 1), (-3, 2), (W + 2, H + 2), (np.nan, 1), (1, np.inf)], F64)])


@pytest.mark.parametrize("s", [1, 3, 8, 300])
@pytest.mark.parametrize("shape", [(65, 130), (1, 7), (5, 1)])
def test_points_on_a_grid_equal_the_statement(ctx, shape, s):
    nodes = G.sample_ref(G.smooth_flow(shape, 15, amp=3.0), s)
    grid = FlowGrid(nodes, s, shape)
    pts = grid_points(shape, s, 16)
    tmat = np.array([[0.98, -0.05, 1.5], [0.05, 0.98, -2.0]])
    img_shape = (max(shape[0] - 2, 1), max(shape[1] - 3, 1))
    _, m, left, top = affine_flow_params(img_shape, F32, shape + (2,), F32, tmat)
    for kw, m6, t6, pad in ((dict(), None, None, (0, 0)), (dict(tmat=tmat, image_shape=img_shape), m, tmat.ravel(), (left, top))):
        exp, ec, ei = G.to_moving_grid_ref(pts, nodes, shape, s, m6, pad)
        got, info = transform_points(pts, grid, "to_moving", return_info=True, **kw)
        assert same_bits(got, exp) and np.array_equal(info.converged, ec.astype(bool)) and np.array_equal(info.inside, ei.astype(bool))
        exp, ec, ei = G.to_reference_grid_ref(pts, nodes, shape, s, t6, pad, 30, 1e-4)
        got, info = transform_points(pts, grid, "to_reference", max_iter=30, tol=1e-4, return_info=True, **kw)
        assert same_bits(got, exp) and np.array_equal(info.converged, ec.astype(bool)) and np.array_equal(info.inside, ei.astype(bool))


def test_points_entry_with_a_separate_output_and_device_nodes(ctx):
    """Context.transform_points writes over its upload (out == pts); the entry with two arrays gives the same"""
    shape, s = (65, 130), 8
    grid = ctx.flow_grid_sample(ctx.asdevice(G.smooth_flow(shape, 17)), s)
    pts = grid_points(shape, s, 18)
    n = len(pts)
    exp = transform_points(pts, grid, "to_reference")
    d_pts, d_out, d_c, d_i = ctx._upload_raw(pts), ctx._raw(n * 16), ctx._raw(n), ctx._raw(n)
    ctx._run(ctx.lib.ma_transform_points_grid, d_pts.ptr, n, grid.nodes.ptr, shape[0], shape[1], s, None, None, 0, 0,
             _lib.MA_POINTS_TO_REFERENCE, 50, 1e-4, d_out.ptr, d_c.ptr, d_i.ptr)
    assert same_bits(ctx.download_raw(d_out, (n, 2), F64), exp)
    assert same_bits(ctx.download_raw(d_pts, (n, 2), F64), pts)


# ---- the Python entries ------------------------------------------------------------------------------------------------------
def test_compress_flow_keeps_the_kind_and_picks_the_statements_stride(ctx):
    shape = (130, 140)
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(F64)
    f = np.stack([5 * np.sin(2 * np.pi * x / 200), 5 * np.cos(2 * np.pi * y / 200)], -1).astype(F32)
    exp_s, exp_maps = FG.choose_stride(lambda s: G.error_maps_ref(f, G.sample_ref(f, s), s, (50, 50), 1 / 32), 1 / 32)
    grid, err = compress_flow(f, cell_size=50, return_error=True)
    assert isinstance(grid, FlowGrid) and isinstance(grid.nodes, np.ndarray) and isinstance(err, FlowGridError)
    assert grid.stride == exp_s == err.stride and same_bits(grid.nodes, G.sample_ref(f, exp_s))
    assert same_bits(err.max_err, exp_maps[0]) and np.array_equal(err.above, exp_maps[1]) and err.invalid.sum() == 0
    assert err.cell_bounds.shape == (3, 3, 4) and err.summary()["max_err"] == err.global_max_err <= 1 / 32
    assert grid.nbytes * exp_s * exp_s < f.nbytes * 1.3
    assert isinstance(grid.expand(), np.ndarray) and same_bits(grid.expand(), G.expand_ref(grid.nodes, shape, exp_s))
    d_grid = compress_flow(ctx.asdevice(f), stride=7)
    assert isinstance(d_grid.nodes, DeviceArray) and isinstance(d_grid.expand(), DeviceArray) and d_grid.stride == 7
    again = flow_grid_error(f, grid, cell_size=50)
    assert same_bits(again.max_err, err.max_err) and again.tol == 1 / 32
    bad = f.copy()
    bad[3, 3, 0] = np.nan
    assert compress_flow(bad).stride == 1
    for call in (lambda: compress_flow(f.astype(F64)), lambda: compress_flow(f, stride=0), lambda: compress_flow(f, tol=-1),
                 lambda: compress_flow(f, tol=float("nan")), lambda: compress_flow(f, cell_size=0),
                 lambda: flow_grid_error(f[:-1], grid), lambda: flow_grid_error(f, f)):
        with pytest.raises(ValueError):
            call()


def test_calls_without_a_grid_path_expand_it_first(ctx):
    shape, s = (65, 130), 8
    f = G.smooth_flow(shape, 19, amp=3.0)
    grid = compress_flow(f, stride=s)
    dense = grid.expand()
    assert same_bits(invert_flow(grid), invert_flow(dense))
    assert same_bits(compose_flows(grid, f), compose_flows(dense, f)) and same_bits(compose_flows(f, grid), compose_flows(f, dense))
    a, b = flow_qc(grid, 40), flow_qc(dense, 40)
    assert same_bits(a.jac_min, b.jac_min) and same_bits(a.flow_mean, b.flow_mean)
    d_grid = FlowGrid(ctx.asdevice(grid.nodes), s, shape)
    assert isinstance(invert_flow(d_grid), DeviceArray)


# ---- the CLI key --------------------------------------------------------------------------------------------------------------
def test_cli_saves_a_grid_per_registered_cycle(ctx, tmp_path):
    H, W = 300, 260
    reg = dict(NumberPyramidLevels=2, NumberIterationsPerLevel=3, TileSize=150, Overlap=30, NumberOfWorkers=0,
               UseFullResImage=True, UseDOG=False)
    ref, mov = synthetic.make_pair(H, W, seed=50, dtype=np.uint16)
    stacks = [np.stack([np.stack([ref, ref // 2])]), np.stack([np.stack([mov, mov // 2])])]      # (C=1, Z=2, H, W)
    paths = {}
    for k, st in enumerate(stacks):
        np.save(tmp_path / f"cyc{k + 1}.npy", st)
        paths[f"Cycle {k + 1}"] = str(tmp_path / f"cyc{k + 1}.npy")
    outs, logs = {}, {}
    for name, extra in (("plain", {}), ("grid", {"SaveFlowGridStride": 8})):
        cfg = {"Input": {"InputImagePaths": paths, "ReferenceCycle": 1, "ReferenceChannel": "0"},
               "Output": {"OutputDir": str(tmp_path / name), "OutputPrefix": "exp_", "SaveOutputToCycleStack": True},
               "RegistrationParameters": {"OptFlowReg": dict(reg, **extra)}}
        (tmp_path / f"{name}.yaml").write_text(yaml.safe_dump(cfg))
        logs[name] = []
        P.run(tmp_path / f"{name}.yaml", log=logs[name].append)
        outs[name] = np.load(tmp_path / name / "exp_optflow_reg_result_stack.npy")
    assert np.array_equal(outs["plain"], outs["grid"])
    assert not list((tmp_path / "plain").glob("*flowgrid*"))
    assert [p.name for p in (tmp_path / "grid").glob("*flowgrid*")] == ["exp_optflow_reg_flowgrid_cyc002.npz"]
    grid = FlowGrid.load(tmp_path / "grid" / "exp_optflow_reg_flowgrid_cyc002.npz")
    assert grid.stride == 8 and grid.shape == (H, W)
    line = [m for m in logs["grid"] if "max_err" in m]
    assert len(line) == 1 and not any("max_err" in m for m in logs["plain"])
    logged = float(re.search(r"max_err ([0-9.eE+-]+|inf|nan) px", line[0]).group(1))
    # the registration the run made, made again: the loaded grid loses against it what the run logged
    r = OptFlowRegistrator()
    r.num_pyr_lvl, r.num_iterations, r.tile_size, r.overlap, r.use_full_res_img, r.use_dog = 2, 3, 150, 30, True, False
    r.ref_img, r.mov_img = max_project_and_normalize(stacks[0][0]), max_project_and_normalize(stacks[1][0])
    flow = r.register()
    assert flow_grid_error(flow, grid).global_max_err <= float(np.float32(logged))      # %.9g gives a float32 back exactly
    w = Warper()
    w.flow = grid
    pages = w.warp_pages([stacks[1][0, 0], stacks[1][0, 1]])
    assert len(pages) == 2 and pages[0].shape == (H, W) and pages[0].dtype == np.uint16 and isinstance(w.flow, FlowGrid)
