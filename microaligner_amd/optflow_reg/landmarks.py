"""Flows from landmark pairs (include/microaligner_landmarks.h): a thin-plate spline fitted on the host in numpy float64 and
evaluated on the device, densely, on the nodes of a FlowGrid, or at points.  No counterpart in the reference.

A pair (r_i, m_i), both (x, y) in pixels, says that the reference-frame point r_i shows what the ORIGINAL moving image
shows at m_i.  With warp(img, f)(p) = img(p - f(p)) the spline is the sampling map s(p) = p - f(p) with s(r_i) = m_i:

    fit  = fit_landmarks(ref_pts, mov_pts, smoothing=0.0)     # host; LandmarkFit
    flow = landmark_flow(fit, shape)                          # (H, W, 2) float32
    grid = landmark_flow(fit, shape, stride=16)               # a FlowGrid
    xy   = landmark_points(fit, pts)                          # where each reference-frame point lies in the moving image

Every argument is checked before any device work.
"""
import numpy as np

from ..device import FlowGrid, get_context, landmark_flow_params, landmark_points_params

MAX_LANDMARKS = 4096           # the fit is O(n^3) on the host
COLLINEAR_REL = 1e-12          # det <= COLLINEAR_REL * trace^2 of the covariance of the normalised centres
SELF_CHECK_PX = 1e-6           # a condition of the fit, not a tolerance (the header, 1. (4))


def tps_kernel(q):
    """U(q) = 0.5 * q * log(q) of squared distances q, U(0) = 0."""
    q = np.asarray(q, np.float64)
    out = np.zeros_like(q)
    pos = q > 0
    out[pos] = (0.5 * q[pos]) * np.log(q[pos])
    return out


class LandmarkFit:
    """The thin-plate spline of n landmark pairs, in the normalised coordinates u = (p - c) * k it was fitted in.

    centres (n, 2): the normalised reference points;  weights (n, 2);  affine (2, 3): row 0 gives s.x, row 1 s.y;
    c (2,), k: the normalisation;  smoothing: in px^2;  residual (n, 2) = m_i - s(r_i);  bending_energy = sum of
    w^T K w over both components;  affine_px (2, 3): the affine part as a matrix that takes reference pixels to moving
    pixels (the M of a two-stage warp), for reporting."""

    def __init__(self, centres, weights, affine, c, k, smoothing, residual, bending_energy):
        self.centres, self.weights, self.affine = centres, weights, affine
        self.c, self.k, self.smoothing = c, float(k), float(smoothing)
        self.residual, self.bending_energy = residual, float(bending_energy)

    def __len__(self):
        return self.centres.shape[0]

    def __repr__(self):
        return (f"LandmarkFit(n={len(self)}, smoothing={self.smoothing:g}, "
                f"residual_rms={float(np.sqrt(np.mean(np.sum(self.residual ** 2, axis=1)))):.3g} px, "
                f"bending_energy={self.bending_energy:.4g})")

    @property
    def affine_px(self):
        lin = self.affine[:, :2] * self.k
        return np.concatenate([lin, (self.affine[:, 2] - lin @ self.c)[:, None]], axis=1)

    @property
    def cw(self):
        """The (n, 4) float64 records (u.x, u.y, w.x, w.y) the kernels read."""
        return np.ascontiguousarray(np.concatenate([self.centres, self.weights], axis=1))

    @property
    def a6(self):
        return np.ascontiguousarray(self.affine.ravel())


def _check_pairs(ref_pts, mov_pts, smoothing):
    try:
        r, m = np.asarray(ref_pts, dtype=np.float64), np.asarray(mov_pts, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"the landmarks must be (n, 2) arrays of numbers: {e}") from None
    if r.ndim != 2 or r.shape[1] != 2 or r.shape != m.shape:
        raise ValueError(f"the landmarks must be two (n, 2) arrays of equal shape, got {r.shape} and {m.shape}")
    if not (np.all(np.isfinite(r)) and np.all(np.isfinite(m))):
        raise ValueError("the landmarks must be finite")
    n = r.shape[0]
    if not 3 <= n <= MAX_LANDMARKS:
        raise ValueError(f"the number of landmark pairs must be in [3, {MAX_LANDMARKS}], got {n}")
    if isinstance(smoothing, bool) or not isinstance(smoothing, (int, float, np.integer, np.floating)):
        raise ValueError(f"smoothing must be a number, got {smoothing!r}")
    smoothing = float(smoothing)
    if not (np.isfinite(smoothing) and smoothing >= 0):
        raise ValueError(f"smoothing must be finite and not negative, got {smoothing!r}")
    return r, m, smoothing


def fit_landmarks(ref_pts, mov_pts, smoothing=0.0):
    """The thin-plate spline through the landmark pairs (ref_pts[i], mov_pts[i]), (n, 2) arrays of (x, y) in pixels with
    3 <= n <= 4096: reference-frame point ref_pts[i] shows what the original moving image shows at mov_pts[i].
    smoothing >= 0, in px^2, trades the fit at the landmarks for less bending (0: interpolation); it is
    scipy.interpolate.RBFInterpolator's for this kernel.  Host only, numpy float64.  ValueError for arrays of the wrong
    shape, non-finite values, collinear landmarks, duplicate reference points without smoothing, a singular system, or
    a fit that misses its own equations by more than 1e-6 px."""
    r, m, smoothing = _check_pairs(ref_pts, mov_pts, smoothing)
    n = r.shape[0]
    c = r.mean(axis=0)
    msd = float(np.mean(np.sum((r - c) ** 2, axis=1)))
    if not (msd > 0 and np.isfinite(msd)):
        raise ValueError("the reference landmarks are collinear (they all coincide)")
    k = 1.0 / np.sqrt(msd)
    u = (r - c) * k
    cov = (u - u.mean(axis=0)).T @ (u - u.mean(axis=0)) / n
    det, trace = cov[0, 0] * cov[1, 1] - cov[0, 1] * cov[1, 0], cov[0, 0] + cov[1, 1]
    if not det > COLLINEAR_REL * trace * trace:
        raise ValueError("the reference landmarks are collinear: a thin-plate spline needs three that are not")
    if smoothing == 0 and np.unique(r, axis=0).shape[0] != n:
        raise ValueError("two reference landmarks are equal: remove one, or fit with smoothing > 0")
    diff = u[:, None, :] - u[None, :, :]
    K = tps_kernel(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1])
    lam = smoothing * k * k
    P = np.concatenate([u, np.ones((n, 1))], axis=1)
    A = np.zeros((n + 3, n + 3))
    A[:n, :n] = K + lam * np.eye(n)
    A[:n, n:] = P
    A[n:, :n] = P.T
    rhs = np.zeros((n + 3, 2))
    rhs[:n] = m
    try:
        sol = np.linalg.solve(A, rhs)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"the landmark system is singular: {e}") from None
    w, a = sol[:n], sol[n:]
    s = K @ w + P @ a
    residual = m - s
    miss = np.abs(residual - lam * w)
    if not (np.all(np.isfinite(sol)) and float(miss.max()) <= SELF_CHECK_PX):
        raise ValueError(f"the landmark fit misses its own equations by {float(np.nanmax(miss)):.3g} px (limit "
                         f"{SELF_CHECK_PX:g}): two reference landmarks nearly coincide, fit with smoothing > 0")
    return LandmarkFit(u, w, np.ascontiguousarray(a.T), c, k, smoothing, residual, float(np.sum(w * (K @ w))))


def _as_fit(fit, smoothing):
    if isinstance(fit, LandmarkFit):
        if smoothing is not None:
            raise ValueError("smoothing belongs to fit_landmarks(): it has no meaning beside a LandmarkFit")
        return fit
    try:
        ref_pts, mov_pts = fit
    except (TypeError, ValueError):
        raise ValueError("expected a LandmarkFit or a pair (ref_pts, mov_pts)") from None
    return fit_landmarks(ref_pts, mov_pts, 0.0 if smoothing is None else smoothing)


def landmark_flow(fit, shape, stride=None, device=False, smoothing=None):
    """The flow of a LandmarkFit (or of a pair (ref_pts, mov_pts), fitted first with `smoothing`) for images of `shape`
    (H, W), evaluated on the device in float64: warp(mov, flow) shows at ref_pts[i] what mov shows at mov_pts[i].
    Without `stride` the dense (H, W, 2) float32 flow, numpy or with device=True a DeviceArray.  With `stride` a FlowGrid of
    that stride whose nodes are the spline at the node positions (numpy nodes, or with device=True device nodes): 1 / stride^2
    of the work; stride=1 is the dense flow held as a FlowGrid."""
    fit = _as_fit(fit, smoothing)
    landmark_flow_params(fit.cw, fit.a6, fit.c, fit.k, shape, 1 if stride is None else stride)
    H, W = int(shape[0]), int(shape[1])
    out = get_context().landmark_flow(fit.cw, fit.a6, fit.c, fit.k, (H, W), 1 if stride is None else stride)
    if not device:
        out = out.numpy()
    return out if stride is None else FlowGrid(out, stride, (H, W))


def landmark_points(fit, points, smoothing=None):
    """Where the reference-frame points `points` ((N, 2) float64, (x, y)) lie in the original moving image according to a
    LandmarkFit (or a pair (ref_pts, mov_pts), fitted first): s(p), evaluated on the device in float64.  A new (N, 2)
    float64 array; a non-finite point gives (NaN, NaN)."""
    fit = _as_fit(fit, smoothing)
    landmark_points_params(fit.cw, fit.a6, fit.c, fit.k, points)
    return get_context().landmark_points(fit.cw, fit.a6, fit.c, fit.k, points)
