"""-m gpu: thin-plate splines of landmark pairs on the device (include/microaligner_landmarks.h).  ma_landmark_points and
ma_landmark_flow against the numpy statement (tests/_landmarks_ref.py) within the derived bound of a float64 chain; the dense
flow, the grid nodes and the points path against each other bit for bit; the sign and frame convention against the
product's own warp and point transform; the model's accuracy as an initialisation; refused arguments."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _landmarks_ref as R  # noqa: E402
from _measured_path import HASH  # noqa: E402
from microaligner_amd import FlowGrid, Warper, _lib, fit_landmarks, landmark_flow, landmark_points, transform_points  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
CHUNK = _lib.MA_LANDMARK_CHUNK
# a block covers 256 columns: 255, 256 and 257 are its edges
SHAPES = [(1, 1), (1, 300), (300, 1), (7, 5), (5, 255), (5, 256), (5, 257), (37, 515), (96, 161), (300, 700)]
COUNTS = sorted({0, 3, 4, 130} | ({CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7} if CHUNK > 1 else set()))
PLACEMENTS = ["integer", "offgrid", "outside"]
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def same_bits(got, exp):
    assert got.dtype == exp.dtype and got.shape == exp.shape
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(got.view(u), exp.view(u))


@functools.lru_cache(maxsize=None)
def synthetic(H, W, n, placement, seed=0):
    """A spline given by its records, not by a fit: n centres placed on integer pixels (a position that meets one takes the
    q == 0 branch), off the grid, or outside the image, weights of mixed sign that bend by a few pixels, and an affine part
    close to the identity in pixels.  (cw, a6, c, k, the centres in pixels)"""
    rng = np.random.default_rng([H, W, n, PLACEMENTS.index(placement), seed])
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0]) + 0.125
    k = 1.0 / max(np.hypot(W - 1, H - 1) / np.sqrt(12.0), 1.0)
    if placement == "integer":
        r = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(F64)
    elif placement == "offgrid":
        r = rng.random((n, 2)) * [max(W - 1, 1), max(H - 1, 1)]
    else:
        side = np.where(rng.random((n, 2)) < 0.5, -1.0, 1.0)
        r = np.array([W - 1, H - 1]) * (0.5 + side * (0.6 + rng.random((n, 2))))
    u = (r - c) * k
    # weights of mixed sign in both components: + - + - ... in x, + + - - ... in y
    i = np.arange(n)
    w = (0.25 + np.abs(rng.normal(0.0, 2.0, (n, 2)))) * np.stack([1.0 - 2.0 * (i % 2), 1.0 - 2.0 * (i // 2 % 2)], axis=1)
    cw = np.ascontiguousarray(np.concatenate([u, w], axis=1))
    a6 = np.array([1.01 / k, 0.02 / k, c[0] + 2.5, -0.015 / k, 0.99 / k, c[1] - 1.75])
    for a in (cw, a6, c, r):
        a.setflags(write=False)
    return cw, a6, c, float(k), r


@functools.lru_cache(maxsize=None)
def statement_flow(H, W, n, placement, stride=1):
    cw, a6, c, k, _ = synthetic(H, W, n, placement)
    flow, bound = R.flow(cw, a6, c, k, H, W, stride)
    flow.setflags(write=False)
    bound.setflags(write=False)
    return flow, bound


def check_flow(ctx, H, W, n, placement, stride=1):
    """the device's grid (stride 1: dense) flow against the statement: the bound of s, plus the rounding to float32"""
    cw, a6, c, k, _ = synthetic(H, W, n, placement)
    exp, bound = statement_flow(H, W, n, placement, stride)
    got = ctx.landmark_flow(cw, a6, c, k, (H, W), stride)
    assert isinstance(got, DeviceArray) and got.dtype == F32 and got.shape == exp.shape
    got = got.numpy().astype(F64)
    assert np.all(np.isfinite(got))
    allowed = bound + 2.0 ** -23 * np.maximum(1.0, np.abs(exp))
    err = np.abs(got - exp)
    print(f"flow {H}x{W} n={n} {placement} stride={stride}: worst error / allowed {(err / allowed).max():.3f}, "
          f"worst allowed {allowed.max():.3g} px")
    assert np.all(err <= allowed)


# ---- 1-4. the kernels against the statement --------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("n", COUNTS)
def test_points_kernel_stays_within_the_derived_bound_of_the_statement(ctx, n, placement):
    """(n + 8) * 2^-53 * (sum |w_i U_i| + |a0 X| + |a1 Y| + |a2|) per component: everything up to q is the same on both
    sides; two logarithms within 1 ulp each (2), the three roundings after the logarithm (3), a sum of n + 3 terms in any
    order against fsum (n + 2), one to spare."""
    worst = 0.0
    for H, W in ((37, 515), (96, 161)):
        cw, a6, c, k, r = synthetic(H, W, n, placement)
        rng = np.random.default_rng(n + 7)
        # positions: on the centres themselves (q == 0), off the grid inside, far outside, and more than one block of them
        p = np.concatenate([r, rng.random((400, 2)) * [W - 1, H - 1], (rng.random((150, 2)) - 0.5) * [8 * W, 8 * H],
                            np.stack(np.meshgrid(np.arange(W, dtype=F64), np.arange(min(H, 3), dtype=F64)), -1).reshape(-1, 2)])
        exp, mag = R.evaluate(cw, a6, c, k, p)
        got = ctx.landmark_points(cw, a6, c, k, p)
        assert got.dtype == F64 and got.shape == p.shape and np.all(np.isfinite(got))
        bound = R.bound(mag, n)
        assert np.all(bound > 0)
        worst = max(worst, float((np.abs(got - exp) / bound).max()))
        print(f"points {H}x{W} n={n} {placement}: worst error / bound {(np.abs(got - exp) / bound).max():.3f}, "
              f"worst bound {bound.max():.3g} px")
        assert np.all(np.abs(got - exp) <= bound)
        if placement == "integer" and n:
            # a position on a centre: that term is exactly zero, whatever its weight
            cw2 = cw.copy()
            cw2[0, 2:] *= 1e6
            assert same_bits(ctx.landmark_points(cw2, a6, c, k, r[:1].copy()), got[:1])
    print(f"points n={n} {placement}: worst error / bound over both frames {worst:.3f}")


def test_a_non_finite_point_gives_nan_and_touches_no_other(ctx):
    cw, a6, c, k, r = synthetic(96, 161, 130, "offgrid")
    p = np.random.default_rng(5).random((300, 2)) * [160, 95]
    clean = ctx.landmark_points(cw, a6, c, k, p)
    bad = p.copy()
    bad[3], bad[64], bad[255], bad[256] = (np.nan, 1.0), (2.0, np.inf), (-np.inf, np.nan), (np.inf, np.inf)
    got = ctx.landmark_points(cw, a6, c, k, bad)
    rows = [3, 64, 255, 256]
    assert np.all(np.isnan(got[rows]))
    keep = np.setdiff1d(np.arange(300), rows)
    assert same_bits(got[keep], clean[keep])
    assert ctx.landmark_points(cw, a6, c, k, np.zeros((0, 2))).shape == (0, 2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_flow_stays_within_the_bound_at_every_shape(ctx, shape):
    H, W = shape
    for placement in PLACEMENTS:
        check_flow(ctx, H, W, 9, placement)


@pytest.mark.parametrize("n", COUNTS)
def test_dense_flow_stays_within_the_bound_at_every_landmark_count(ctx, n):
    for (H, W), placement in zip(((37, 515), (96, 161), (7, 5)), PLACEMENTS):
        check_flow(ctx, H, W, n, placement)
    check_flow(ctx, 37, 515, n, "integer", stride=7)


# ---- 5. the paths agree bit for bit ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(H, W, n=40, smoothing=0.0):
    rng = np.random.default_rng([H, W, n])
    ny = max(1, int(round(np.sqrt(n * H / W))))
    nx = -(-n // ny)
    cy, cx = np.divmod(rng.permutation(ny * nx)[:n], nx)
    r = np.stack([(cx + 0.25 + 0.5 * rng.random(n)) * max(W - 1, 2) / nx, (cy + 0.25 + 0.5 * rng.random(n)) * max(H - 1, 2) / ny],
                 axis=1)
    m = r @ np.array([[1.01, 0.02], [-0.015, 0.99]]) + [2.5, -1.75] + rng.normal(0, 1.5, (n, 2))
    return fit_landmarks(r, m, smoothing)


@pytest.mark.parametrize("shape", [(37, 515), (96, 161), (1, 300), (300, 1), (5, 257), (7, 5), (1, 1), (130, 66)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_grid_nodes_equal_the_dense_flow_bit_for_bit(ctx, shape):
    """(96, 161) at stride 16 ends on a node, (37, 515) has a short last interval on both axes, (130, 66) at 64 one of a
    single pixel; 64 is larger than (7, 5), (5, 257)'s height and (1, 1)."""
    H, W = shape
    f = fitted(H, W)
    dense = landmark_flow(f, shape)
    assert isinstance(dense, np.ndarray) and dense.dtype == F32 and dense.shape == (H, W, 2)
    for s in (1, 2, 7, 16, 64):
        grid = landmark_flow(f, shape, stride=s)
        assert isinstance(grid, FlowGrid) and grid.stride == s and grid.shape == (H, W) and isinstance(grid.nodes, np.ndarray)
        ys = np.minimum(np.arange(R.grid_nodes(H, s)) * s, H - 1)
        xs = np.minimum(np.arange(R.grid_nodes(W, s)) * s, W - 1)
        assert same_bits(grid.nodes, np.ascontiguousarray(dense[ys][:, xs])), s


@pytest.mark.parametrize("shape", [(37, 515), (96, 161), (1, 300), (5, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_flow_equals_the_points_path_bit_for_bit(ctx, shape):
    H, W = shape
    f = fitted(H, W)
    dense = landmark_flow(f, shape)
    p = R.node_positions(H, W, 1)
    s = landmark_points(f, p)
    assert s.dtype == F64 and s.shape == p.shape
    assert same_bits(dense, (p - s).astype(F32).reshape(H, W, 2))
    assert same_bits(landmark_flow(f, shape), dense) and same_bits(landmark_points(f, p), s)        # two calls, the same bits


def test_device_results_hold_the_same_bits_and_feed_the_warp_and_the_point_transform(ctx):
    H, W = 96, 161
    f = fitted(H, W)
    dense, grid = landmark_flow(f, (H, W)), landmark_flow(f, (H, W), stride=16)
    d_dense, d_grid = landmark_flow(f, (H, W), device=True), landmark_flow(f, (H, W), stride=16, device=True)
    assert isinstance(d_dense, DeviceArray) and isinstance(d_grid, FlowGrid) and isinstance(d_grid.nodes, DeviceArray)
    assert same_bits(d_dense.numpy(), dense) and same_bits(d_grid.nodes.numpy(), grid.nodes)
    # a pair of point sets is fitted first and gives what its fit gives
    rng = np.random.default_rng(2)
    r = rng.random((12, 2)) * [W - 1, H - 1]
    m = r + rng.normal(0, 1.0, (12, 2))
    assert same_bits(landmark_flow((r, m), (H, W)), landmark_flow(fit_landmarks(r, m), (H, W)))
    assert same_bits(landmark_flow((r, m), (H, W), smoothing=10.0), landmark_flow(fit_landmarks(r, m, 10.0), (H, W)))
    # the grid is an ordinary FlowGrid: the warp and the point transform take it, on the host or on the device
    img = np.random.default_rng(3).integers(0, 60000, (H, W)).astype(np.uint16)
    outs = []
    for g in (grid, d_grid):
        w = Warper()
        w.image, w.flow = img, g
        outs.append(w.warp())
    assert outs[0].shape == (H, W) and np.array_equal(outs[0], outs[1]) and outs[0].any()
    p = rng.random((50, 2)) * [W - 1, H - 1]
    via_grid = transform_points(p, grid, "to_moving")
    assert same_bits(via_grid, transform_points(p, d_grid, "to_moving"))
    # on its nodes the grid holds the spline itself, rounded to float32: p - node = s(p) within 2^-24 |flow|
    q = R.node_positions(H, W, 16)
    s = landmark_points(f, q)
    assert np.all(np.abs(transform_points(q, grid, "to_moving") - s) <= 2.0 ** -23 * np.maximum(1.0, np.abs(q - s)))


# ---- 6. the sign and frame convention ---------------------------------------------------------------------------------------------
def test_the_flow_shows_at_each_reference_landmark_what_the_moving_image_shows_at_its_partner(ctx):
    """Integer reference landmarks r_i on 96 x 161 and an image that holds its own x (then y) coordinate: the whole-image warp
    through the landmark flow reads m_i.x (m_i.y) at r_i within the warp's 1/32 px coordinate quantum plus the float32
    rounding of the flow, and transform_points takes r_i to m_i.  A reversed sign or swapped roles miss by twice the
    displacement, here several pixels."""
    H, W = 96, 161
    gy, gx = np.meshgrid(np.arange(8, H - 8, 16), np.arange(10, W - 10, 20), indexing="ij")
    r = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(F64)
    m = r + np.stack([4.0 * np.sin(r[:, 1] / 23.0) + 2.25, -3.0 * np.cos(r[:, 0] / 31.0) + 0.5 * r[:, 1] / H], axis=1)
    assert np.abs(m - r).max(axis=0).min() > 3 and m.min() >= 1 and np.all(m <= [W - 2, H - 2])
    flow = landmark_flow((r, m), (H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    ix, iy = r[:, 0].astype(int), r[:, 1].astype(int)
    for axis, ramp in ((0, xx), (1, yy)):
        w = Warper()
        w.image, w.flow, w.tmat = ramp.astype(F32), flow, IDENTITY
        out = w.warp()
        err = np.abs(out[iy, ix].astype(F64) - m[:, axis])
        print(f"warp of the {'xy'[axis]} ramp at the landmarks: max error {err.max():.4f} px")
        assert np.all(err <= 1.0 / 32 + 2.0 ** -23 * W)
    got = transform_points(r, flow, "to_moving")
    print("transform_points at the landmarks: max error", np.abs(got - m).max())
    assert np.all(np.abs(got - m) <= 2.0 ** -23 * max(W, H))
    assert np.all(np.abs(landmark_points((r, m), r) - m) <= 1e-6)


# ---- 7. the model as an initialisation ----------------------------------------------------------------------------------------------
def true_flow(p, H, W):
    """a smooth deformation of a few pixels"""
    x, y = p[:, 0], p[:, 1]
    return np.stack([3.0 * np.sin(2 * np.pi * x / (1.7 * W)) * np.cos(np.pi * y / (2.0 * H)) + 1.5,
                     2.0 * np.cos(2 * np.pi * x / (2.3 * W) + 0.4) + 1.25 * np.sin(np.pi * y / (1.3 * H))], axis=1)


@pytest.mark.parametrize("shape, lattice", [((96, 161), (8, 12)), ((37, 515), (4, 30))], ids=["96x161", "37x515"])
def test_landmarks_on_a_lattice_recover_a_smooth_deformation(ctx, shape, lattice):
    """The dense flow against the analytic flow the landmarks were read from stays within 4 x the error of the statement on the
    same inputs (the project's margin for accuracy tables).  Statement: 0.0295 px on 96 x 161 with 8 x 12 landmarks, 0.0467 px
    on 37 x 515 with 4 x 30, for a flow of up to 4.5 px."""
    H, W = shape
    gy, gx = np.meshgrid(np.linspace(0, H - 1, lattice[0]), np.linspace(0, W - 1, lattice[1]), indexing="ij")
    r = np.stack([gx.ravel(), gy.ravel()], axis=1)
    m = r - true_flow(r, H, W)
    p = R.node_positions(H, W, 1)
    want = true_flow(p, H, W).reshape(H, W, 2)
    ref = R.fit(r, m)
    stated, _ = R.flow(*R.records(ref), ref["c"], ref["k"], H, W)
    e_cpu = np.abs(stated - want).max()
    e_gpu = np.abs(landmark_flow((r, m), shape).astype(F64) - want).max()
    print(f"{H}x{W}, {r.shape[0]} landmarks: statement {e_cpu:.4f} px, device {e_gpu:.4f} px")
    assert 0 < e_cpu < 0.1
    assert e_gpu <= 4 * e_cpu


# ---- 8. the C entries refuse what the header says ---------------------------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments_without_launching(ctx):
    cw, a6, c, k, _ = synthetic(7, 5, 4, "offgrid")
    lib, h = ctx.lib, ctx.handle
    d_cw = ctx._upload_raw(cw)
    sentinel = np.full((7, 5, 2), 7.0, F32)
    out = ctx.asdevice(sentinel.copy())
    pts = np.full((6, 2), 3.0)
    d_pts = ctx._upload_raw(pts)
    A = (C.c_double * 6)(*a6)

    def bad6(i, v):
        b = a6.copy()
        b[i] = v
        return (C.c_double * 6)(*b)
    ok = dict(cw=d_cw.ptr, n=4, a6=A, cx=c[0], cy=c[1], k=k, H=7, W=5, stride=1, out=out.ptr)
    for kw in (dict(cw=None), dict(a6=None), dict(out=None), dict(n=-1), dict(n=(1 << 20) + 1), dict(H=0), dict(W=0), dict(H=-3),
               dict(H=(1 << 24) + 1), dict(W=(1 << 24) + 1), dict(stride=0), dict(stride=-2), dict(a6=bad6(0, np.nan)),
               dict(a6=bad6(5, np.inf)), dict(cx=np.nan), dict(cy=-np.inf), dict(k=np.inf), dict(k=np.nan)):
        assert lib.ma_landmark_flow(h, *dict(ok, **kw).values()) == _lib.MA_EINVAL, kw
        assert b"invalid argument" in lib.ma_last_error()
    assert lib.ma_landmark_flow(None, *ok.values()) == _lib.MA_EINVAL
    okp = dict(cw=d_cw.ptr, n=4, a6=A, cx=c[0], cy=c[1], k=k, pts=d_pts.ptr, m=6, out=d_pts.ptr)
    for kw in (dict(cw=None), dict(a6=None), dict(pts=None), dict(out=None), dict(n=-1), dict(n=(1 << 20) + 1), dict(m=-1),
               dict(a6=bad6(2, np.nan)), dict(cx=np.inf), dict(cy=np.nan), dict(k=-np.inf)):
        assert lib.ma_landmark_points(h, *dict(okp, **kw).values()) == _lib.MA_EINVAL, kw
    assert lib.ma_landmark_points(None, *okp.values()) == _lib.MA_EINVAL
    ctx.sync()
    assert same_bits(out.numpy(), sentinel)                                    # no refused call wrote anything
    assert same_bits(ctx.download_raw(d_pts, (6, 2), F64), pts)
    # the same arguments, unchanged, are accepted
    assert lib.ma_landmark_flow(h, *ok.values()) == _lib.MA_OK
    assert lib.ma_landmark_points(h, *okp.values()) == _lib.MA_OK
    ctx.sync()
    assert not same_bits(out.numpy(), sentinel)
    assert same_bits(ctx.download_raw(d_pts, (6, 2), F64), ctx.landmark_points(cw, a6, c, k, pts))      # out may be pts


def test_the_loaded_library_is_this_trees():
    from microaligner_amd import build
    assert _lib.source_hash() == build.source_hash() == HASH
    assert hasattr(_lib.load(), "ma_landmark_flow") and hasattr(_lib.load(), "ma_landmark_points")
