"""Refining a flow on the CPU (no GPU): the numpy float32 statement of include/microaligner_flowrefine.h
(tests/_flow_refine_ref.py) against an independent float64 one; its accuracy on an analytic pair whose true flow is exact;
what the floor does on glass; the statement's properties; and the argument checks of the entry points before any device
work."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_refine_ref as R  # noqa: E402
import _texture_ref as T  # noqa: E402
from _remap_interp_ref import InterpRef  # noqa: E402
from _warp_compose_ref import warp_affine_flow  # noqa: E402

F32, F64 = np.float32, np.float64
SIZES = [(96, 161), (37, 515)]
QUANTUM = 1.0 / 32            # of the warp's coordinates
BOUND_F64 = 337               # 4 x 84.26, the worst case of test_one_step_against_a_float64_statement
# The floor of the glass tests as a multiple of the median lam_min of the glass.  A floor AT the glass's lam_min only
# halves a step that noise drives (the system's matrix there is about lam_min on its diagonal, so adding as much again
# divides the solution by two): the drift on glass is the unregularised one over about 1 + K for a floor of K lam_min.
# Unregularised the drift after 6 steps is 0.7 - 0.8 px (measured below, and the figure the feature was proposed with), so
# that 0.05 px with the test's margin of 4 asks for 0.75 / (1 + K) <= 0.0125: K >= 59.  64 is a factor of 6 below the
# lam_min of the pair's texture (2.5 against 15.6 squared grey levels), whose accuracy it does not change (below).
FLOOR_FACTOR = 64.0


@pytest.fixture(scope="module")
def interp(tmp_path_factory):
    return InterpRef(tmp_path_factory.mktemp("remap_interp_ref"))


def taps_of_radius(r):
    sigma = r / 3.0
    taps = R.gaussian_taps(sigma, (r - 0.5) / sigma)         # ceil(r - 0.5) = r whatever the rounding of the product
    assert len(taps) == r + 1
    return taps


def epe(flow, truth, margin=16):
    """median endpoint error `margin` px inside"""
    d = np.hypot(flow[..., 0] - truth[..., 0], flow[..., 1] - truth[..., 1])
    return float(np.median(d[margin:-margin, margin:-margin]))


def smoothed_truth(truth):
    """what a wide window leaves of the true flow: a Gaussian of sigma 15 over it"""
    from scipy.ndimage import gaussian_filter
    return np.stack([gaussian_filter(truth[..., k], 15.0, mode="nearest") for k in (0, 1)], -1).astype(F32)


# ---- one step against float64 ----------------------------------------------------------------------------------------------
def step_f64(ref, wp, taps, floor, weight=None):
    from scipy.ndimage import correlate1d
    I, Rf = wp.astype(F64), np.asarray(ref).astype(F64)
    H, W = I.shape
    xs, ys = np.arange(W), np.arange(H)
    gx = 0.5 * (I[:, np.minimum(xs + 1, W - 1)] - I[:, np.maximum(xs - 1, 0)])
    gy = 0.5 * (I[np.minimum(ys + 1, H - 1), :] - I[np.maximum(ys - 1, 0), :])
    w = np.ones((H, W)) if weight is None else np.where(weight > 0, weight, 0).astype(F64)
    e = I - Rf
    k = np.concatenate([taps[:0:-1], taps]).astype(F64)
    sxx, sxy, syy, sxe, sye = (correlate1d(correlate1d(p, k, axis=1, mode="constant"), k, axis=0, mode="constant")
                               for p in (w * gx * gx, w * gx * gy, w * gy * gy, w * gx * e, w * gy * e))
    a, c = sxx + float(floor), syy + float(floor)
    det = a * c - sxy * sxy
    return np.stack([(c * sxe - sxy * sye) / det, (a * sye - sxy * sxe) / det], -1)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("r", [1, 3, 12, 21, 49])
def test_one_step_against_a_float64_statement(r, weighted):
    """The float32 statement's step from a zero flow (so that the result is the step itself) against
    scipy.ndimage.correlate1d(mode="constant") in float64 with the same float32 taps, on the 96 x 161 analytic pair (ref
    against the unwarped moving image), floor 2.5, no clamp; weighted: weights that are 0 at 30 % of the pixels and 0.75
    elsewhere.  Measured max |d32 - d64| / (2^-24 max|d64|):
        plain:    r = 1: 84.26, r = 3: 53.12, r = 12: 22.52, r = 21: 19.69, r = 49: 18.18
        weighted: r = 1: 43.83, r = 3: 35.81, r = 12: 18.81, r = 21: 14.19, r = 49: 17.07
    (max|d64| = 2.9 px at r = 1, 0.78 px at r = 12, 0.18 px at r = 49).  The error is that of the 2 x 2 solve, which
    amplifies the rounding of the sums by the system's condition; small windows are the worst conditioned.
    Bound: 4 x the worst observed: 337 x 2^-24 max|d64|."""
    ref, mov, _ = R.analytic_pair(96, 161)
    taps = taps_of_radius(r)
    weight = None
    if weighted:
        weight = (np.where(np.random.default_rng(1).random((96, 161)) < 0.3, 0, 1) * 0.75).astype(F32)
    out, stats = R.step(ref, mov, np.zeros((96, 161, 2), F32), taps, 2.5, weight, max_step=1e30)
    assert stats.invalid == 0 and stats.clamped == 0
    d64 = step_f64(ref, mov, taps, 2.5, weight)
    unit = 2.0 ** -24 * float(np.abs(d64).max())
    err = float(np.abs(out.astype(F64) - d64).max()) / unit
    print(f"r = {r} {'weighted' if weighted else 'plain'}: max |d32 - d64| = {err:.2f} x 2^-24 max|d| (max|d| = "
          f"{np.abs(d64).max():.3f} px)")
    assert err <= BOUND_F64



# ---- accuracy on the analytic pair -----------------------------------------------------------------------------------------
FLOOR = 2.5     # squared grey levels: FLOOR_FACTOR x the glass's lam_min of test_the_floor_holds_glass_still (0.039)
# median endpoint error in px 16 px inside after 6 steps of sigma 4, measured with the float32 statement: (start, after)
MEASURED_EPE = {((96, 161), "zero"): (0.5315, 0.0492), ((96, 161), "wide"): (0.4964, 0.0475),
                ((37, 515), "zero"): (0.6206, 0.0522), ((37, 515), "wide"): (0.5687, 0.0493)}


@pytest.mark.parametrize("start", ["zero", "wide"])
@pytest.mark.parametrize("shape", SIZES)
def test_six_steps_reach_the_true_flow_of_the_analytic_pair(interp, shape, start):
    """ref(p) = I(p - f(p)) and mov = I, I a sum of ten cosines with periods of 6 - 40 px evaluated at the displaced
    coordinates, so that f (0.8 px amplitude, 48 px period) is the exact flow.  From a zero flow and from f smoothed with
    sigma 15 (what a wide window leaves), 6 steps of sigma 4 at floor 2.5.  Median endpoint error 16 px inside, measured
    (MEASURED_EPE): 96 x 161: zero 0.531 -> 0.049, wide 0.496 -> 0.048; 37 x 515: zero 0.621 -> 0.052, wide 0.569 ->
    0.049.  What is left is mostly the bilinear warp's own error on the short periods (the warped image has lost contrast
    that the reference has, by an amount that depends on the sub-pixel position), besides its 1/32 px coordinate quantum.
    Bound: 4 x the measured value, never more than a quarter of the start's median."""
    ref, mov, truth = R.analytic_pair(*shape)
    flow = np.zeros(shape + (2,), F32) if start == "zero" else smoothed_truth(truth)
    before = epe(flow, truth)
    out, stats, _ = R.refine(interp, ref, mov, flow, FLOOR, num_iter=6)
    after = epe(out, truth)
    print(f"{shape} {start}: median endpoint error {before:.4f} -> {after:.4f} px; step_max {[round(s.step_max, 3) for s in stats]}, "
          f"clamped {[s.clamped for s in stats]}, invalid {[s.invalid for s in stats]}")
    m_before, m_after = MEASURED_EPE[shape, start]
    assert abs(before - m_before) < 5e-4
    assert after <= min(4 * m_after, 0.25 * before)
    assert all(s.invalid == 0 for s in stats)


# ---- glass -----------------------------------------------------------------------------------------------------------------
MEASURED_GLASS = {(96, 161): 0.0138, (37, 515): 0.0132}       # median |flow| on glass in px after 6 steps at FLOOR_FACTOR lam_min


@pytest.mark.parametrize("shape", SIZES)
def test_the_floor_holds_glass_still(interp, shape):
    """The analytic pair with its left third replaced by the constant 128 plus independent noise of sigma 0.3 in each image.
    The floor comes from the region as texture_maps gives it: the median lam_min (same window) of the glass at least r px
    from the tissue, times FLOOR_FACTOR (see there for why not 1).  Median |flow| on that glass after 6 steps from a zero
    flow, measured (MEASURED_GLASS): 96 x 161: 0.0138 px (lam_min 0.0391, floor 2.50); 37 x 515: 0.0132 px (lam_min
    0.0360, floor 2.30).  Bound: 4 x that, capped at 0.05 px.  With floor = 1e-3 -- in effect unregularised -- it is
    0.768 and 0.827 px, and must exceed ten times the bound: the regulariser is what holds it.  For the record, with the
    lam_min itself as the floor (factor 1) it is 0.404 and 0.420 px: half the unregularised drift, as the factor's
    derivation says.  The tissue's accuracy is that of the pair without glass (0.050 and 0.051 px)."""
    ref, mov, truth, n = R.glass_pair(*shape)
    taps = R.gaussian_taps(4.0)
    r = len(taps) - 1
    lam_min, _ = T.eigenvalues(ref, taps)
    glass = (slice(None), slice(0, n - r))
    base = float(np.median(lam_min[glass]))

    def drift(floor):
        out, stats, _ = R.refine(interp, ref, mov, None, floor, num_iter=6)
        assert all(s.invalid == 0 for s in stats)
        return float(np.median(np.hypot(out[glass][..., 0], out[glass][..., 1]))), out

    held, out = drift(FLOOR_FACTOR * base)
    free, _ = drift(1e-3)
    at_noise, _ = drift(base)
    tissue = epe(out[:, n + r:], truth[:, n + r:])
    print(f"{shape}: lam_min of the glass {base:.4f}, floor {FLOOR_FACTOR * base:.3f}: median |flow| on glass {held:.4f} px; "
          f"floor 1e-3: {free:.4f} px; floor = lam_min: {at_noise:.4f} px; tissue endpoint error {tissue:.4f} px")
    bound = min(4 * MEASURED_GLASS[shape], 0.05)
    assert held <= bound
    assert free > 10 * bound
    assert tissue <= 4 * MEASURED_EPE[shape, "zero"][1]


# ---- properties ------------------------------------------------------------------------------------------------------------
SMOOTH = (24.0, 64.0)       # periods in px of the pair that the true flow aligns to within the warp's quantum


@pytest.mark.parametrize("shape", SIZES)
def test_a_flow_that_aligns_the_pair_moves_by_less_than_a_warp_quantum(interp, shape):
    """A step from the true flow, 16 px inside (the warp's zero fill at the border reaches r + 2 = 14 px in), moves no
    component by 1/32 px -- on a pair that the flow does align under the warp the step uses: cosines with periods of
    24 - 64 px, where the median residual |Wp - R| (0.04 - 0.05 grey levels) is below what a shift by one quantum makes
    (median |g| / 32 = 0.09 - 0.11), which the test checks first.  Measured: 0.0248 px on both sizes.
    The pair of the accuracy test does not meet that premise: with periods down to 6 px the bilinear warp leaves a median
    residual of 0.47 - 0.50 grey levels at the true flow, twice a quantum's worth (0.25), and one step from the true flow
    moves up to 0.047 / 0.041 px; further steps go on to the fixed point that the accuracy test finds 0.05 px (median)
    from the truth.  Printed for the record, not asserted."""
    inner = (slice(16, -16), slice(16, -16))
    moved = {}
    for periods in (SMOOTH, (6.0, 40.0)):
        ref, mov, truth = R.analytic_pair(*shape, periods=periods)
        start = truth.astype(F32)
        wp = warp_affine_flow(interp, mov, start, R.IDENTITY, "linear")
        gx, gy = R.gradients(wp)
        residual, quantum_worth = float(np.median(np.abs(wp - ref)[inner])), float(np.median(np.hypot(gx, gy)[inner])) * QUANTUM
        out, stats = R.step(ref, wp, start, R.gaussian_taps(4.0), FLOOR)
        moved[periods] = float(np.abs(out[inner] - start[inner]).max())
        print(f"{shape} periods {periods}: median |Wp - R| {residual:.3f}, median |g| / 32 {quantum_worth:.3f}; a step from the "
              f"true flow moves at most {moved[periods]:.4f} px inside")
        assert (residual < quantum_worth) == (periods == SMOOTH) and stats.invalid == 0
    assert moved[SMOOTH] < QUANTUM


def random_case(H, W, seed=3):
    rng = np.random.default_rng(seed)
    ref, mov, _ = R.analytic_pair(H, W, seed)
    flow = rng.normal(0, 2, (H, W, 2)).astype(F32)
    return ref, mov, flow, rng


def test_a_weight_of_zero_everywhere_returns_the_flow_bit_for_bit():
    ref, mov, flow, _ = random_case(40, 70)
    for weight in (np.zeros((40, 70), F32), np.zeros((40, 70), np.uint8), np.full((40, 70), np.nan, F32),
                   np.full((40, 70), -1, F32), np.full((40, 70), np.inf, F32)):
        out, stats = R.step(ref, mov, flow, R.gaussian_taps(2.0), 2.5, weight)
        assert np.array_equal(out.view(np.uint32), flow.view(np.uint32))
        assert stats == R.Stats(0.0, 0, 0)


@pytest.mark.parametrize("max_step", [0.25, 0.03])
def test_max_step_bounds_every_step(interp, max_step):
    ref, mov, _ = R.analytic_pair(96, 161)
    taps = R.gaussian_taps(4.0)
    free, s_free = R.step(ref, mov, np.zeros((96, 161, 2), F32), taps, FLOOR)
    out, s = R.step(ref, mov, np.zeros((96, 161, 2), F32), taps, FLOOR, None, max_step)
    over = (np.abs(free) > F32(max_step)).any(-1)
    assert s_free.clamped == 0 and 0 < over.sum() < over.size           # hit on some pixels and not on others
    assert s.clamped == int(over.sum()) and s.step_max == float(F32(max_step)) and s.invalid == 0
    assert np.array_equal(out, np.clip(free, -F32(max_step), F32(max_step)))
    _, stats, _ = R.refine(interp, ref, mov, None, FLOOR, num_iter=4, max_step=max_step)
    assert all(st.step_max <= float(F32(max_step)) for st in stats) and stats[0].clamped > 0


def test_a_uint8_mask_equals_its_float_map():
    ref, mov, flow, rng = random_case(40, 70)
    mask = (rng.random((40, 70)) < 0.6).astype(np.uint8) * 255
    a, sa = R.step(ref, mov, flow, R.gaussian_taps(2.0), 2.5, mask)
    b, sb = R.step(ref, mov, flow, R.gaussian_taps(2.0), 2.5, (mask != 0).astype(F32))
    plain, _ = R.step(ref, mov, flow, R.gaussian_taps(2.0), 2.5)
    assert np.array_equal(a, b) and sa == sb and not np.array_equal(a, plain)


def test_bad_pixels_drop_out_and_a_nan_flow_stays_nan():
    """a NaN or Inf pixel of either image takes itself and (through the gradients of the warped image) its four neighbours
    out of every sum; the steps stay finite.  A NaN in the flow stays a NaN and takes no part in the step's statistics."""
    ref, mov, flow, _ = random_case(40, 70)
    ref[5, 6], ref[30, 60], mov[20, 33], mov[0, 0] = np.nan, np.inf, np.nan, -np.inf
    flow[7, 7, 0], flow[8, 9, 1] = np.nan, np.inf
    out, stats = R.step(ref, mov, flow, R.gaussian_taps(2.0), 2.5)
    bad = ~np.isfinite(out)
    assert bad.sum() == 2 and bad[7, 7, 0] and bad[8, 9, 1] and stats.invalid == 0 and np.isfinite(stats.step_max)
    # the same as a weight of 0 on those pixels of clean images
    clean_ref, clean_mov = np.nan_to_num(ref, nan=1.0, posinf=1.0, neginf=1.0), np.nan_to_num(mov, nan=1.0, posinf=1.0, neginf=1.0)
    P, Q = R.products(ref, mov), R.products(clean_ref, clean_mov)
    drop = np.zeros((40, 70), bool)
    for y, x in ((5, 6), (30, 60)):
        drop[y, x] = True
    for y, x in ((20, 33), (0, 0)):
        drop[max(y - 1, 0):y + 2, x] = True
        drop[y, max(x - 1, 0):x + 2] = True
    for p, q in zip(P, Q):
        assert not p[drop].any() and np.array_equal(p[~drop], q[~drop])


def test_the_loop_stops_after_a_step_within_tol(interp):
    ref, mov, _ = R.analytic_pair(37, 515)
    full, stats, converged = R.refine(interp, ref, mov, None, FLOOR, num_iter=6)
    assert len(stats) == 6 and not converged
    tol = sorted(s.step_max for s in stats)[2]                 # the third smallest: some step is the first within it
    first = next(k for k, s in enumerate(stats) if s.step_max <= tol)
    out, early, converged = R.refine(interp, ref, mov, None, FLOOR, num_iter=6, tol=tol)
    assert converged and len(early) == first + 1 and early == stats[:first + 1] and first < 5
    again, _, _ = R.refine(interp, ref, mov, None, FLOOR, num_iter=first + 1)
    assert np.array_equal(out, again)


def test_the_loops_warp_is_the_one_resampling_warp(interp):
    """one step of the loop is the statement's step on warp_affine_flow of the float32 moving image, smaller than the
    reference and padded, through a matrix"""
    ref, mov, _ = R.analytic_pair(40, 70)
    small = mov[2:-3, 4:-5].astype(F32)
    a = np.deg2rad(2.0)
    tmat = np.array([[np.cos(a), -np.sin(a), 1.5], [np.sin(a), np.cos(a), -0.75]])
    flow = np.random.default_rng(0).normal(0, 0.5, (40, 70, 2)).astype(F32)
    out, stats, _ = R.refine(interp, ref, small, flow, FLOOR, tmat=tmat, num_iter=1, sigma=2.0)
    wp = warp_affine_flow(interp, small, flow, tmat, "linear")
    assert wp.shape == (40, 70) and wp.dtype == F32
    exp, s = R.step(ref, wp, flow, R.gaussian_taps(2.0), FLOOR)
    assert np.array_equal(out, exp) and stats == [s]


# ---- argument checks -------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_c_entry_raises_before_any_device_work():
    from microaligner_amd import _lib, device
    from microaligner_amd.device import flow_refine_step_params as P
    H, W = 20, 30
    ok = dict(ref=np.zeros((H, W), np.uint16), warped=np.zeros((H, W), F32), flow=np.zeros((H, W, 2), F32),
              taps=R.gaussian_taps(1.0), floor=2.5)
    got = P(**ok)
    assert got[:3] == (H, W, _lib.MA_U16) and got[4:] == (3, 2.5, _lib.MA_SMOOTH_WEIGHT_NONE, 1.0)
    assert P(**dict(ok, weight=np.ones((H, W), F32)))[6] == _lib.MA_SMOOTH_WEIGHT_F32
    assert P(**dict(ok, weight=np.ones((H, W), np.uint8), max_step=0.5))[6:] == (_lib.MA_SMOOTH_WEIGHT_U8, 0.5)
    for bad in (dict(ref=None), dict(ref=np.zeros((H, W), F64)), dict(ref=np.zeros((H, W + 1), np.uint8)),
                dict(ref=np.zeros((H, W, 1), np.uint8)), dict(warped=None), dict(warped=np.zeros((H, W), np.uint8)),
                dict(warped=np.zeros((W, H), F32)), dict(flow=None), dict(flow=np.zeros((H, W, 2), F64)),
                dict(flow=np.zeros((H, W), F32)), dict(flow=np.zeros((H, W, 3), F32)),
                dict(taps=None), dict(taps=np.ones(130, F32)), dict(taps=np.zeros(4, F32)), dict(taps=np.array([0.5], F32)),
                dict(taps=np.array([0.5, np.nan], F32)), dict(taps=np.array([0.5, -0.1], F32)),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=1e-50),
                dict(floor=1e40), dict(floor="1"), dict(floor=True), dict(floor=None),
                dict(max_step=0.0), dict(max_step=-1.0), dict(max_step=float("inf")), dict(max_step=float("nan")),
                dict(max_step=None),
                dict(weight=[[1.0]]), dict(weight=np.ones((H, W), F64)), dict(weight=np.ones((H, W + 1), F32)),
                dict(weight=np.ones((2, 3), F32)), dict(weight=np.ones((H, W), bool))):
        with pytest.raises(ValueError):
            P(**dict(ok, **bad))
    big = object.__new__(device.DeviceArray)      # sides are checked on the shape alone
    big.shape, big.dtype = ((1 << 24) + 1, 2, 2), np.dtype(F32)
    with pytest.raises(ValueError):
        P(**dict(ok, flow=big))
    big.ptr = big.ctx = None             # nothing for __del__ to free


def test_refine_flow_refuses_its_own_arguments_before_any_device_work(monkeypatch):
    import microaligner_amd
    from microaligner_amd.optflow_reg import flow_refine
    monkeypatch.setattr(flow_refine, "get_context", lambda: pytest.fail("a refused call reached the device"))
    H, W = 20, 30
    ref, mov, flow = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint16), np.zeros((H, W, 2), F32)
    with pytest.raises(TypeError):
        flow_refine.refine_flow(ref, mov, flow)                      # floor is required
    with pytest.raises(TypeError):
        flow_refine.refine_flow(ref, mov, flow, 2.5)                 # and is a keyword
    for bad in (dict(floor=0.0), dict(floor=float("nan")), dict(floor=None), dict(sigma=0.0), dict(sigma=50.0),
                dict(sigma=43.0), dict(truncate=-1.0), dict(sigma="4"), dict(num_iter=0), dict(num_iter=2.0),
                dict(num_iter=True), dict(tol=-1.0), dict(tol=float("nan")), dict(tol="0"), dict(max_step=0.0),
                dict(max_step=float("inf")), dict(labels="u8"), dict(labels=1), dict(tmat=np.eye(3)),
                dict(tmat=[[1, 0, 0], [0, 1, np.nan]]), dict(weight=np.ones((H, W), F64)), dict(weight=np.ones((2, 2), F32)),
                dict(ref_img=np.zeros((H, W), F64)), dict(ref_img=None), dict(mov_img=np.zeros((H + 1, W), np.uint8)),
                dict(mov_img=np.zeros((H, W, 3), np.uint8)), dict(mov_img=[[1]]), dict(flow=np.zeros((H, W, 2), F64)),
                dict(flow=np.zeros((H, W + 1, 2), F32)), dict(flow=np.zeros((H, W), F32)), dict(flow=[[0.0]]),
                dict(flow=microaligner_amd.FlowGrid(np.zeros((3, 3, 2), F32), 16, (H + 1, W)))):
        kw = dict(dict(ref_img=ref, mov_img=mov, flow=flow, floor=2.5), **bad)
        with pytest.raises(ValueError):
            flow_refine.refine_flow(kw.pop("ref_img"), kw.pop("mov_img"), kw.pop("flow"), **kw)
    assert {"refine_flow", "FlowRefineInfo"} <= set(microaligner_amd.__all__)
    assert microaligner_amd.refine_flow is flow_refine.refine_flow
