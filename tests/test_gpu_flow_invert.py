"""-m gpu: the flow inverse and the point transforms on the device.  ma_invert_flow and ma_transform_points against the
numpy statements of include/microaligner_flowinvert.h (tests/_flow_invert_ref.py) bit for bit; to_moving against the
product's own warp through tmat and the flow; the entry points; refused arguments."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_invert_ref as R  # noqa: E402
from microaligner_amd import Warper, _lib, compose_flows, invert_flow, transform_points  # noqa: E402
from microaligner_amd.device import DeviceArray, affine_flow_params  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64

# the shape list of the composition's tests
SHAPES = [(1, 1), (1, 300), (300, 1), (40, 255), (40, 256), (40, 257), (13, 64), (9, 700), (7, 5), (2049, 1031)]


def same_bits(got, exp):
    """equal as bit patterns, any NaN payload standing for NaN"""
    assert got.dtype == exp.dtype and got.shape == exp.shape
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(got.view(u)[~gn], exp.view(u)[~en])


def make_flow(H, W, kind):
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    if kind == "folding":            # runs to max_iter in the folds
        return np.stack([12 * np.sin(x / 9), 4 * np.cos(y / 5)], -1).astype(F32)
    if kind == "integers":           # the samples fall on pixels: -c in two steps
        f = np.empty((H, W, 2), F32)
        f[...] = (3.0, -7.0)
        return f
    f = np.stack([3 * np.sin(x / 17) + 2 * np.cos(y / 23), 2.5 * np.cos(x / 13 + y / 31)], -1).astype(F32)
    if kind == "non_finite":
        for k, v in enumerate(((np.nan, 1.0), (np.inf, -np.inf), (-np.inf, np.nan), (1e30, -1e30), (2.0, np.nan))):
            f[(5 + 11 * k) % H, (6 + 37 * k) % W] = v
    return f


def check_dense(ctx, f, max_iter, tol):
    exp, exp_res, exp_missed, _ = R.invert_flow_ref(f, max_iter, tol)
    got, info = ctx.invert_flow(ctx.asdevice(f), max_iter, tol, return_info=True)
    assert same_bits(got.numpy(), exp)
    assert same_bits(info.residual.numpy(), exp_res)
    assert info.not_converged == exp_missed
    return exp_missed


@pytest.mark.parametrize("kind", ["smooth", "folding", "integers", "non_finite"])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_numpy_statement_bit_for_bit(ctx, shape, kind):
    missed = check_dense(ctx, make_flow(*shape, kind), 25, 1e-3)
    if kind == "folding" and shape[1] >= 255:
        assert missed > 0
    if kind in ("smooth", "integers"):
        assert missed == 0


@pytest.mark.parametrize("max_iter, tol", [(1, 1e-3), (1, 0.0), (7, 0.0), (40, 0.0), (3, 1e-1), (40, 1e-6)])
@pytest.mark.parametrize("kind", ["smooth", "folding", "integers", "non_finite"])
def test_kernel_equals_the_statement_at_one_step_and_at_zero_tolerance(ctx, kind, max_iter, tol):
    for shape in ((67, 301), (1, 1), (130, 64)):
        check_dense(ctx, make_flow(*shape, kind), max_iter, tol)


def test_inverse_undoes_the_flow_on_the_device(ctx):
    """compose_flows(f, invert_flow(f)) ~ 0 within the bound of tests/test_flow_invert_ref.py, on the device's own
    composition; and the call without info enqueues the same result."""
    f = R.analytic_flow("B")
    g, info = invert_flow(f, max_iter=60, tol=1e-3, return_info=True)
    assert isinstance(g, np.ndarray) and info.not_converged == 0 and isinstance(info.residual, np.ndarray)
    assert info.residual.shape == f.shape[:2] and info.residual.max() <= F32(1e-3)
    got = float(np.abs(compose_flows(f, g)).max())
    bound = R.lipschitz(f) * (1 / 64 + 1e-3) + 1e-4
    print(f"max |compose_flows(f, invert_flow(f))| = {got:.5f} px, bound {bound:.5f} px")
    assert got <= bound
    assert same_bits(invert_flow(f, max_iter=60, tol=1e-3), g)


def test_entry_points_take_numpy_and_device_arrays(ctx):
    f = make_flow(150, 333, "smooth")
    exp, exp_res, exp_missed, _ = R.invert_flow_ref(f, 50, 1e-3)
    out = invert_flow(f)
    assert isinstance(out, np.ndarray) and same_bits(out, exp)
    dout = invert_flow(ctx.asdevice(f))
    assert isinstance(dout, DeviceArray) and dout.shape == f.shape and same_bits(dout.numpy(), exp)
    dout, info = invert_flow(ctx.asdevice(f), return_info=True)
    assert isinstance(dout, DeviceArray) and isinstance(info.residual, DeviceArray) and info.not_converged == exp_missed
    assert same_bits(info.residual.numpy(), exp_res)
    pts = points(1000, 150, 333, 5)
    exp_p = R.to_reference_ref(pts, f, max_iter=50, tol=1e-4)
    for flow in (f, ctx.asdevice(f)):                       # flow numpy or device resident, points numpy in and out
        got = transform_points(pts, flow, "to_reference")
        assert isinstance(got, np.ndarray) and got.dtype == F64 and same_bits(got, exp_p[0])
        got, pinfo = ctx.transform_points(pts, flow, "to_reference", return_info=True)
        assert same_bits(got, exp_p[0]) and pinfo.converged.dtype == bool and pinfo.inside.dtype == bool
        assert np.array_equal(pinfo.converged, exp_p[1].astype(bool)) and np.array_equal(pinfo.inside, exp_p[2].astype(bool))


# ---- points ---------------------------------------------------------------------------------------------------------------
TMAT = np.array([[np.cos(np.deg2rad(3.0)) * 1.01, -np.sin(np.deg2rad(3.0)) * 1.01, 7.5],
                 [np.sin(np.deg2rad(3.0)) * 1.01, np.cos(np.deg2rad(3.0)) * 1.01, -4.25]])


def points(n, H, W, seed):
    """points inside and up to 40 px outside the image, integer and half-integer ones, and non-finite ones"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-40, W + 40, n), rng.uniform(-40, H + 40, n)], -1)
    if n >= 16:
        p[0:4] = np.rint(p[0:4])
        p[4:8] = np.rint(p[4:8]) + 0.5
        p[8], p[9], p[10] = (0.0, 0.0), (W - 1.0, H - 1.0), (W - 1.0 + 1e-9, 3.0)
        p[11], p[12], p[13], p[14] = (np.nan, 3.0), (5.0, np.inf), (-np.inf, np.nan), (1e300, -1e300)
    return p


@pytest.mark.parametrize("n", [0, 1, 100003])
@pytest.mark.parametrize("with_tmat", [False, True])
@pytest.mark.parametrize("direction", ["to_moving", "to_reference"])
@pytest.mark.parametrize("kind", ["smooth", "folding"])
def test_points_equal_the_float64_statement_bit_for_bit(ctx, kind, direction, with_tmat, n):
    H, W = 300, 420
    f = make_flow(H, W, kind)
    pts = points(n, H, W, n + 1)
    shape, tmat, m6, pad = None, None, None, (0, 0)
    if with_tmat:
        shape, tmat = (H - 21, W - 10), TMAT
        _, m6, left, top = affine_flow_params(shape, F32, f.shape, f.dtype, tmat)
        pad = (left, top)
        assert pad == (5, 10)
    if direction == "to_moving":
        exp = R.to_moving_ref(pts, f, m6, pad)
    else:
        exp = R.to_reference_ref(pts, f, None if tmat is None else tmat.ravel(), pad, 30, 1e-4)[:3]
    got, info = ctx.transform_points(pts, ctx.asdevice(f), direction, tmat=tmat, image_shape=shape, max_iter=30, tol=1e-4,
                                     return_info=True)
    assert got.shape == (n, 2) and info.converged.shape == (n,) and info.inside.shape == (n,)
    assert same_bits(got, exp[0])
    assert np.array_equal(info.converged, exp[1].astype(bool)) and np.array_equal(info.inside, exp[2].astype(bool))
    if n > 16:
        assert np.isnan(got[11:14]).all() and not info.converged[11:14].any() and not info.inside[11:14].any()
        assert 0 < info.inside.mean() < 1
        if direction == "to_reference":
            assert info.converged[:8].all() if kind == "smooth" else not info.converged.all()


def test_to_moving_is_the_coordinate_the_warp_samples_at(ctx):
    """An image that holds its own x (then y) coordinate, warped by Warper through tmat (a 3 degree similarity) and a
    smooth flow with linear interpolation, reads back the coordinate it was sampled at: a linear ramp is interpolated
    exactly up to cv2's quantisation of the coordinate to 1/32 px (at most 1/64 px off) and the float32 rounding of
    coordinates below max(h, w) (2^-23 max(h, w) for the map and the interpolation).  Wherever the sample lies inside
    the moving image, so that all four taps do, it equals transform_points(grid, "to_moving"): sign, channel order,
    tmat and padding against the product's own warp."""
    H, W, h, w = 500, 640, 479, 630
    f = (R.analytic_flow("A", (H, W)) * F32(1.5)).astype(F32)
    ys, xs = np.mgrid[0:H, 0:W]
    grid = np.stack([xs.ravel(), ys.ravel()], -1).astype(F64)
    moving, info = transform_points(grid, f, "to_moving", tmat=TMAT, image_shape=(h, w), return_info=True)
    assert info.converged.all() and info.inside.all()
    mx, my = moving[:, 0].reshape(H, W), moving[:, 1].reshape(H, W)
    taps_inside = (mx >= 0) & (mx <= w - 1) & (my >= 0) & (my <= h - 1)
    assert 0.8 < taps_inside.mean() < 1
    iy, ix = np.mgrid[0:h, 0:w].astype(F32)
    bound = 1 / 64 + 2.0 ** -23 * max(h, w)
    for ramp, coord, name in ((ix, mx, "x"), (iy, my, "y")):
        wr = Warper()
        wr.image, wr.flow, wr.tmat, wr.interpolation = np.ascontiguousarray(ramp), f, TMAT, "linear"
        warped = wr.warp()
        assert warped.shape == (H, W) and warped.dtype == F32
        err = float(np.abs(warped.astype(F64) - coord)[taps_inside].max())
        print(f"{name}: max |warp(ramp) - to_moving| = {err:.5f} px, bound {bound:.5f} px")
        assert err <= bound


def test_spots_and_masks_follow_the_registration(ctx):
    """the two uses: points of the moving frame carried into the registered frame land where the warp puts their
    pixels; a mask of the registered frame warped by the inverse flow lands in the moving frame."""
    H, W = 400, 520
    f = R.analytic_flow("A", (H, W))
    g, info = invert_flow(f, return_info=True)
    assert info.not_converged == 0
    spots = np.array([[100.0, 120.0], [300.25, 200.5], [411.0, 333.0]])
    reg, pinfo = transform_points(spots, f, "to_reference", return_info=True)
    assert pinfo.converged.all() and pinfo.inside.all()
    back = transform_points(reg, f, "to_moving")
    assert np.abs(back - spots).max() <= R.lipschitz(f) * 1e-4 + 1e-9
    # q - g(q) solves the same equation at integer q as to_reference (tests/test_flow_invert_ref.py has the bound)
    L = R.lipschitz(f)
    q = np.array([[100.0, 120.0], [411.0, 333.0]])
    dense = q - g[[120, 333], [100, 411]].astype(F64)
    assert np.abs(dense - transform_points(q, f, "to_reference")).max() <= (L * 1.1e-3 + 8 * 2.0 ** -24 * W) / (1 - L)
    # a labelled disc of the registered frame, carried into the moving frame by the nearest warp with the inverse flow
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (np.hypot(xx - 260, yy - 200) <= 60).astype(np.uint16) * 7
    wr = Warper()
    wr.image, wr.flow, wr.interpolation, wr.tile_size, wr.overlap = mask, g, "nearest", 1000, 100
    moved = wr.warp()
    # a pixel s of the moving frame belongs to the disc iff to_reference(s) does; leave 1.5 px at the rim to rounding
    s = np.stack([xx.ravel(), yy.ravel()], -1).astype(F64)
    r = np.hypot(*(transform_points(s, f, "to_reference") - (260, 200)).T).reshape(H, W)
    assert np.array_equal(moved[r <= 58.5], np.full((r <= 58.5).sum(), 7, np.uint16)) and not moved[r >= 61.5].any()
    assert set(np.unique(moved)) == {0, 7}


# ---- refused arguments ------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_c_entries(ctx):
    f = make_flow(50, 60, "smooth")
    d, out, res = ctx.asdevice(f), ctx.empty(f.shape, F32), ctx.empty(f.shape[:2], F32)
    H, W, big = 50, 60, (1 << 24) + 1
    inv = lambda *a: ctx._run(ctx.lib.ma_invert_flow, *a)
    for args in ((None, H, W, 5, 1e-3, out.ptr, res.ptr, None), (d.ptr, H, W, 5, 1e-3, None, res.ptr, None),
                 (d.ptr, 0, W, 5, 1e-3, out.ptr, None, None), (d.ptr, H, 0, 5, 1e-3, out.ptr, None, None),
                 (d.ptr, -1, W, 5, 1e-3, out.ptr, None, None), (d.ptr, big, 1, 5, 1e-3, out.ptr, None, None),
                 (d.ptr, 1, big, 5, 1e-3, out.ptr, None, None), (d.ptr, H, W, 0, 1e-3, out.ptr, None, None),
                 (d.ptr, H, W, -3, 1e-3, out.ptr, None, None), (d.ptr, H, W, 5, -1e-3, out.ptr, None, None),
                 (d.ptr, H, W, 5, float("nan"), out.ptr, None, None), (d.ptr, H, W, 5, float("inf"), out.ptr, None, None),
                 (d.ptr, H, W, 5, 1e-3, d.ptr, None, None)):          # out == flow
        with pytest.raises(ValueError):
            inv(*args)
    assert ctx.lib.ma_invert_flow(None, d.ptr, H, W, 5, 1e-3, out.ptr, None, None) == _lib.MA_EINVAL
    assert ctx.lib.ma_invert_flow(ctx.handle, d.ptr, H, W, 5, -1.0, out.ptr, None, None) == _lib.MA_EINVAL
    assert same_bits(d.numpy(), f)                                    # a refused call wrote nothing

    n = 10
    p = ctx._upload_raw(points(16, H, W, 1)[:n])
    o, cv, ins = ctx._raw(n * 16), ctx._raw(n), ctx._raw(n)
    bad6 = (C.c_double * 6)(1, 0, float("nan"), 0, 1, 0)
    tp = lambda *a: ctx._run(ctx.lib.ma_transform_points, *a)
    ok = dict(pts=p.ptr, n=n, flow=d.ptr, H=H, W=W, m6=None, t6=None, left=0, top=0, direction=1, max_iter=5, tol=1e-4,
              out=o.ptr, conv=cv.ptr, ins=ins.ptr)
    tp(*ok.values())
    for kw in (dict(pts=None), dict(flow=None), dict(out=None), dict(conv=None), dict(ins=None), dict(n=-1), dict(H=0),
               dict(W=0), dict(H=big), dict(W=big), dict(m6=bad6), dict(t6=bad6), dict(left=-1), dict(top=-1),
               dict(direction=2), dict(direction=-1), dict(max_iter=0), dict(tol=-1.0), dict(tol=float("nan")),
               dict(tol=float("inf"))):
        with pytest.raises(ValueError):
            tp(*dict(ok, **kw).values())
    assert ctx.lib.ma_transform_points(None, *ok.values()) == _lib.MA_EINVAL
    assert ctx.lib.ma_transform_points(ctx.handle, *dict(ok, direction=7).values()) == _lib.MA_EINVAL


def test_the_loaded_library_is_this_trees_and_its_hash_ignores_the_new_source():
    from microaligner_amd import build
    assert _lib.source_hash() == build.source_hash()
    assert "flow_invert.hip" in build.SOURCES and "microaligner_flowinvert.h" not in " ".join(build.HEADERS)
