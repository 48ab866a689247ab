"""The numpy float32 statement of include/microaligner_flowrefine.h: the products, the two smoothing passes, the solve, the
clamp, the add and the three statistics of one step, and the loop of refine_flow() around it.  numpy rounds every float32
operation on its own and keeps denormals, which is the arithmetic the header asks of the kernels, so the kernels must give
these bits (the sign and payload of a NaN apart).  The loop's warp is tests/_warp_compose_ref.warp_affine_flow on
tests/_remap_interp_ref.InterpRef, the CPU restatement of cv2.remap that the warp tests use."""
import collections

import numpy as np

from _flow_smooth_ref import fir, gaussian_taps, pixel_weight

F32, F64 = np.float32, np.float64
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
Stats = collections.namedtuple("Stats", "step_max clamped invalid")


def gradients(wp):
    """(gx, gy) of the float32 image wp: central differences with a replicated border"""
    H, W = wp.shape
    xs, ys = np.arange(W), np.arange(H)
    with np.errstate(all="ignore"):
        gx = F32(0.5) * (wp[:, np.minimum(xs + 1, W - 1)] - wp[:, np.maximum(xs - 1, 0)])
        gy = F32(0.5) * (wp[np.minimum(ys + 1, H - 1), :] - wp[np.maximum(ys - 1, 0), :])
    return gx, gy


def products(ref, wp, weight=None):
    """(P0 .. P4) of the header, zeros at every pixel that is not live"""
    assert wp.dtype == F32 and ref.shape == wp.shape
    R = np.asarray(ref).astype(F32)
    w = pixel_weight(weight, wp.shape)
    gx, gy = gradients(wp)
    with np.errstate(all="ignore"):
        live = np.isfinite(w) & (w > 0) & np.isfinite(wp) & np.isfinite(R) & np.isfinite(gx) & np.isfinite(gy)
        a, b, e = w * gx, w * gy, wp - R
        return [np.where(live, p, F32(0)).astype(F32) for p in (a * gx, a * gy, b * gy, a * e, b * e)]


def step(ref, wp, flow, taps, floor, weight=None, max_step=1.0):
    """(flow + d, Stats) of one step"""
    assert flow.dtype == F32 and taps.dtype == F32
    floor, max_step = F32(floor), F32(max_step)
    with np.errstate(all="ignore"):
        sxx, sxy, syy, sxe, sye = (fir(fir(p, taps, 1), taps, 0) for p in products(ref, wp, weight))
        a, c = sxx + floor, syy + floor
        det = a * c - sxy * sxy
        dx, dy = (c * sxe - sxy * sye) / det, (a * sye - sxy * sxe) / det
        good = np.isfinite(det) & (det > 0) & np.isfinite(dx) & np.isfinite(dy)
        dx, dy = np.where(good, dx, F32(0)).astype(F32), np.where(good, dy, F32(0)).astype(F32)
        cx, cy = np.clip(dx, -max_step, max_step), np.clip(dy, -max_step, max_step)
        clamped = (cx != dx) | (cy != dy)
        out = np.stack([flow[..., 0] + cx, flow[..., 1] + cy], -1).astype(F32)
    step_max = float(max(np.abs(cx).max(), np.abs(cy).max()))
    return out, Stats(step_max, int(clamped.sum()), int((~good).sum()))


def refine(interp, ref, mov, flow, floor, tmat=None, sigma=4.0, truncate=3.0, num_iter=3, tol=0.0, max_step=1.0, weight=None):
    """(flow, list of Stats, converged): the loop of refine_flow(); interp: an InterpRef.  ref and mov are the images the
    steps see (the labels, for labels="dog")."""
    from _warp_compose_ref import warp_affine_flow
    taps = gaussian_taps(sigma, truncate)
    tmat = IDENTITY if tmat is None else tmat
    mov32 = np.asarray(mov).astype(F32)
    flow = np.zeros(ref.shape + (2,), F32) if flow is None else flow
    stats, converged = [], False
    for _ in range(num_iter):
        wp = warp_affine_flow(interp, mov32, flow, tmat, "linear")
        flow, s = step(ref, wp, flow, taps, floor, weight, max_step)
        stats.append(s)
        if s.step_max <= tol:
            converged = True
            break
    return flow, stats, converged


# ---- the analytic pair of the accuracy tests -------------------------------------------------------------------------------
def cosine_image(x, y, seed=0, n=10, periods=(6.0, 40.0)):
    """n cosines with periods of 6 - 40 px in random directions, evaluated at the float64 coordinates (x, y): grey levels
    around 128 with a standard deviation of 24"""
    rng = np.random.default_rng(seed)
    v = np.zeros_like(x, dtype=F64)
    for _ in range(n):
        period, theta, phase = rng.uniform(*periods), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        k = 2 * np.pi / period
        v += np.cos(k * (np.cos(theta) * x + np.sin(theta) * y) + phase)
    return 128.0 + 60.0 * v / np.sqrt(n / 2.0) / 2.5


def true_flow(H, W, amplitude=0.8, period=48.0):
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    k = 2 * np.pi / period
    return np.stack([amplitude * np.sin(k * y + 0.3) * np.cos(k * x / 1.3), amplitude * np.cos(k * x + 1.1) * np.sin(k * y / 1.7)], -1)


def analytic_pair(H, W, seed=0, periods=(6.0, 40.0)):
    """(ref, mov, flow) float32, float32, float64: mov = I on the grid and ref(p) = I(p - f(p)) with I = cosine_image and
    f = true_flow.  The warp reads mov at p - flow(p), so f is the exact flow, up to the warp's interpolation."""
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    f = true_flow(H, W)
    mov = cosine_image(x, y, seed, periods=periods)
    ref = cosine_image(x - f[..., 0], y - f[..., 1], seed, periods=periods)
    return ref.astype(F32), mov.astype(F32), f


def glass_pair(H, W, seed=0, noise=0.3):
    """analytic_pair with the left third of both images replaced by a constant plus independent noise of sigma `noise`;
    -> (ref, mov, flow, number of glass columns)"""
    ref, mov, f = analytic_pair(H, W, seed)
    n = W // 3
    rng = np.random.default_rng(seed + 100)
    ref[:, :n] = (128.0 + rng.normal(0, noise, (H, n))).astype(F32)
    mov[:, :n] = (128.0 + rng.normal(0, noise, (H, n))).astype(F32)
    return ref, mov, f, n
