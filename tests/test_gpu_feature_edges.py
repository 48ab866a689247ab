"""-m gpu: the feature stage (csrc/daisy.hip: FAST, keypoint selection, window cutting, DAISY over content rectangles,
compaction, ma_feature_extract) at chunk, capacity, window and tiny-image edges.  Cases and expectations come from
tests/test_feature_edges_ref.py, which checks on the CPU that they are right and that they meet the boundaries they claim;
the reference is the oracle (oracle/feature_oracle.py), the host-cut windows and numpy's stable selection -- never another
device call -- and every comparison is np.array_equal."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_feature_edges_ref as R  # noqa: E402
from microaligner_amd.feature_reg import feature_detection as FD  # noqa: E402
from microaligner_amd.feature_reg.sparse_cpu import Daisy  # noqa: E402

pytestmark = pytest.mark.gpu
TABLES = FD._daisy_tables(Daisy(radius=21, q_radius=3, q_theta=8, q_hist=8))


# ---- 1. selection ----------------------------------------------------------------------------------------------------------
def _check_selection(ctx, cases):
    """fast_keypoints over the cases' tiles in ONE call (same interior, limit and threshold) against each expectation."""
    c0 = cases[0]
    assert all((c.Pi, c.limit, c.threshold, c.margin) == (c0.Pi, c0.limit, c0.threshold, c0.margin) for c in cases)
    stack = np.ascontiguousarray(np.stack([c.tile for c in cases]))
    counts, kp = ctx.fast_keypoints(ctx.asdevice(stack), c0.margin, c0.limit, threshold=c0.threshold)
    assert kp.shape == (len(cases), c0.limit, 3)
    for t, c in enumerate(cases):
        bad = R.selection_mismatch(counts[t], kp[t], c.expected, c.n, c.limit)
        assert bad is None, (c.name, bad)


@pytest.mark.parametrize("n", R.COUNT_NS)
def test_corner_count_against_the_capacity(ctx, n):
    """0 .. 8193 corners of mixed scores at limit = 8192 (KS_CAP): fewer corners than the limit, exactly as many, one more."""
    _check_selection(ctx, [R.count_case(n)])


@pytest.mark.parametrize("limit", [1, R.N_LIMIT - 1, R.N_LIMIT, R.N_LIMIT + 1])
def test_limit_against_the_corner_count(ctx, limit):
    _check_selection(ctx, [R.limit_case(limit)])


@pytest.mark.parametrize("name", R.TIE_CASES)
def test_ties_at_the_cut(ctx, name):
    """All corners equal; a cut exactly between two score levels (need_eq == 0 with s* > 0); one tie taken; all ties but one;
    cuts at score 1 and at score 254; threshold 100 (corners of value <= 100 vanish)."""
    _check_selection(ctx, [R.tie_case(name)])


@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_last_tie_at_thread_chunk_and_wave_boundaries(ctx, name):
    """The last tie taken sits just before / just behind a multiple of 16 (a collecting thread's scores) or of 4096 (a chunk)
    in row-major index, or in the final, partial chunk of a 403^2 interior."""
    _check_selection(ctx, [R.edge_case(name)])


@pytest.mark.parametrize("name", R.BIG_CASES)
def test_more_than_256_chunks(ctx, name):
    """A 1040^2 interior is 265 chunks: kp_cut_kernel walks them in two passes and carries the running counts of ties
    (all_equal) and of the whole selection (two_levels) into the second, where the cut falls."""
    _check_selection(ctx, [R.big_case(name)])


@pytest.mark.parametrize("limit", [R.KS_CAP, 100])
@pytest.mark.parametrize("reverse", [False, True])
def test_several_tiles_in_one_call(ctx, limit, reverse):
    """An all-zero tile, a constant one, two corners, 8464 equal corners and 8193 mixed ones in one call, in that order and
    reversed: the per-tile offsets into the key lists, the chunk histograms and the chunk bases."""
    tiles, maps = R.multi_tiles()
    order = range(len(tiles))[::-1] if reverse else range(len(tiles))
    stack = np.ascontiguousarray(np.stack([tiles[t] for t in order]))
    counts, kp = ctx.fast_keypoints(ctx.asdevice(stack), 3, limit)
    for k, t in enumerate(order):
        n = int((maps[t] > 0).sum())
        bad = R.selection_mismatch(counts[k], kp[k], R.expected_selection(maps[t], limit), n, limit)
        assert bad is None, (t, bad)


@pytest.mark.parametrize("Pi,margin", R.NMS_CASES)
def test_score_maps_at_block_edges_and_below_the_ring(ctx, Pi, margin):
    """ma_fast_nms at interiors of 255, 256, 257 (a thread per x, 256 per block) and of 1, 6, 7 px (7: one scorable pixel)."""
    tile, exp = R.nms_case(Pi, margin)
    got = ctx.fast_nms(ctx.asdevice(np.ascontiguousarray(tile[None])), margin)
    assert got.shape == (1, Pi, Pi) and np.array_equal(got[0], exp)


# ---- 2. windows and descriptors --------------------------------------------------------------------------------------------
def _extract(ctx, d_img, limit, workspace_bytes=0, wait=True):
    desc, pts, resp, n = ctx.feature_extract(d_img, R.TILE, R.OV, limit, *TABLES, workspace_bytes=workspace_bytes, wait=wait)
    if not wait:
        ctx.sync()
        n = int(n[0])
    return (ctx.download_raw(pts, (n, 2), np.float64), ctx.download_raw(resp, (n,), np.int32),
            ctx.download_raw(desc, (n, 200), np.float32))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _windows_equal_the_host_cut(ctx, d_img, exp):
    got = ctx.cut_tiles(d_img, R.TILE, R.OV, 0, len(exp.windows)).numpy()
    assert np.array_equal(got, np.stack(exp.windows))


def _run_dense(ctx):
    """A call that fills the cubes of 16 windows: what it leaves beyond the content of a later, smaller call must not count."""
    img, _ = R.dense_case()
    return _extract(ctx, ctx.asdevice(img), 12)


@pytest.mark.parametrize("shape", R.SINGLE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_window_images(ctx, shape):
    """Images smaller than a tile: content of 3 .. 63 px, whose rectangle dilated by the halos 1, 12, 30 is 63, 64 or 65 wide
    (a column block of the smoothing), narrower than a halo, one pixel, one row, one column.  Points, responses and every
    descriptor against the oracle; the same bits directly after a call that filled the workspace with 16 dense windows, and
    on a second run."""
    img, exp = R.single_case(shape)
    d_img = ctx.asdevice(img)
    _windows_equal_the_host_cut(ctx, d_img, exp)
    first = _extract(ctx, d_img, R.LIMIT)
    bad = R.features_mismatch(first, exp)
    assert bad is None, bad
    _run_dense(ctx)
    after = _extract(ctx, d_img, R.LIMIT)
    bad = R.features_mismatch(after, exp)
    assert bad is None, "after a dense call: " + bad
    assert _same(_extract(ctx, d_img, R.LIMIT), after)


@pytest.mark.parametrize("shape", [(40, 61), (63, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_whole_tile_entry_equals_the_window_route(ctx, shape):
    """ma_daisy_describe on the host-cut window (every rectangle the whole tile) at the same points."""
    img, exp = R.single_case(shape)
    assert len(exp.pts) >= 3
    window = np.ascontiguousarray(exp.windows[0][None])
    got = ctx.daisy_describe(ctx.asdevice(window), np.zeros(len(exp.pts), np.int32), exp.pts, *TABLES)
    assert np.array_equal(got, exp.desc)
    assert np.array_equal(got, _extract(ctx, ctx.asdevice(img), R.LIMIT)[2])


def test_window_route_at_the_largest_limit(ctx):
    """limit = 8192 (KS_CAP) through ma_feature_extract: every corner of the window is kept and compacted."""
    img, exp = R.capacity_case()
    bad = R.features_mismatch(_extract(ctx, ctx.asdevice(img), R.KS_CAP), exp)
    assert bad is None, bad


@pytest.mark.parametrize("shape", R.REMAINDER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_last_row_and_column_remainders(ctx, shape):
    """The last tile row / column holds 1, 50, 51, 52, 99 or 100 px: below 51 the window before it ends in zeros."""
    img, exp = R.remainder_case(shape)
    d_img = ctx.asdevice(img)
    _windows_equal_the_host_cut(ctx, d_img, exp)
    bad = R.features_mismatch(_extract(ctx, d_img, 12), exp)
    assert bad is None, bad


def test_both_smoothing_schedules_over_ragged_rectangles(ctx):
    """16 windows with ragged content in one batch (32 outputs per thread), in batches of two and of one (16 outputs per
    thread): each equal to the oracle, hence to each other."""
    img, exp = R.dense_case()
    d_img = ctx.asdevice(img)
    _windows_equal_the_host_cut(ctx, d_img, exp)
    P = R.TILE + 2 * R.OV
    runs = [_extract(ctx, d_img, 12, workspace_bytes=k * 128 * P * P) for k in (0, 1, 2)]
    for got in runs:
        bad = R.features_mismatch(got, exp)
        assert bad is None, bad
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2])


@pytest.mark.parametrize("limit", R.DROP_LIMITS)
def test_dropped_windows_at_batch_edges(ctx, limit):
    """Windows with 0, 1 and 2 corners (dropped) and with 3 (kept) first and last of a batch, at batch sizes one, two and all;
    a limit equal to a window's corner count, one less, and one that drops every window; the enqueue-only route."""
    img, exp = R.drop_image(), R.drop_case(limit)
    d_img = ctx.asdevice(img)
    P = R.TILE + 2 * R.OV
    _windows_equal_the_host_cut(ctx, d_img, exp)
    _run_dense(ctx)
    for k in (0, 1, 2):
        got = _extract(ctx, d_img, limit, workspace_bytes=k * 128 * P * P)
        bad = R.features_mismatch(got, exp)
        assert bad is None, (k, bad)
        assert _same(_extract(ctx, d_img, limit, workspace_bytes=k * 128 * P * P, wait=False), got)


# ---- 3. FeatureRegistrator on tiny images --------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("tile", [1000, 100])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("shape", R.TINY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_feature_registrator_on_tiny_images(shape, dtype, tile, levels):
    """register() on images below every pyramid level (the full-resolution image is the only level: use_full_res_img, as
    test_register_and_warp_on_tiny_images does for the dense stage), feature stage on the device against `features_on_host`
    (sparse_cpu.py, the statement the kernels reproduce): the same matrix bit for bit and the same log, or the same exception
    type."""
    from microaligner_amd import FeatureRegistrator
    ref, mov = R.tiny_pair(shape, dtype)
    out = []
    for host in (False, True):
        f = FeatureRegistrator()
        f.num_pyr_lvl, f.num_iterations, f.tile_size, f.use_full_res_img = levels, 2, tile, True
        f.features_on_host = host
        f.ref_img, f.mov_img = ref, mov
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                T = f.register()
        except Exception as e:   # noqa: BLE001
            T = type(e)
        out.append((T, buf.getvalue()))
    (dev, log_dev), (host, log_host) = out
    assert type(dev) is type(host), (dev, host)
    if isinstance(dev, type):
        assert dev is host
    else:
        assert dev.shape == (2, 3) and np.array_equal(dev, host), (dev, host)
    assert log_dev == log_host
    assert "Pyramid factor 1" in log_dev or isinstance(dev, type)


@pytest.mark.parametrize("shape", [(60, 60), (151, 201)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_feature_registrator_without_a_level_fails_alike(shape):
    """Below 200 px a side no pyramid level is kept, and without use_full_res_img none is left: the reference multiplies an empty
    list of matrices (feature_registrator.py:115, :218) and fails with an IndexError; so do both routes here."""
    from microaligner_amd import FeatureRegistrator
    ref, mov = R.tiny_pair(shape, np.uint8)
    raised = []
    for host in (False, True):
        f = FeatureRegistrator()
        f.verbose, f.num_pyr_lvl, f.features_on_host = False, 2, host
        f.ref_img, f.mov_img = ref, mov
        with pytest.raises(Exception) as e:
            f.register()
        raised.append(e.type)
    assert raised == [IndexError, IndexError]
