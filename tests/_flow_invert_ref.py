"""CPU statements of include/microaligner_flowinvert.h in numpy, one array operation per rounding:
(a) invert_flow_ref: the dense inverse in float32;
(b) to_moving_ref / to_reference_ref: the point transforms in float64;
and the analytic test flows with their Lipschitz constants.  TEST INFRASTRUCTURE, not product code."""
import numpy as np

F32, F64 = np.float32, np.float64


def sample(f, mx, my, dt):
    """S(f; mx, my) for 1-D coordinate arrays of dtype dt: (n, 2) of dtype dt.  The taps are converted to dt, every
    operation is one array operation in dt and so rounded on its own."""
    H, W = f.shape[:2]
    assert mx.dtype == dt and my.dtype == dt
    with np.errstate(invalid="ignore", over="ignore"):
        cx = np.fmin(np.fmax(mx, dt(0)), dt(W - 1))         # fmax / fmin return the other operand for a NaN
        cy = np.fmin(np.fmax(my, dt(0)), dt(H - 1))
        x0, y0 = np.floor(cx), np.floor(cy)
        ax, ay = (cx - x0)[:, None], (cy - y0)[:, None]
        bx, by = dt(1) - ax, dt(1) - ay
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
        v00, v01, v10, v11 = (f[iy, ix].astype(dt), f[iy, ix1].astype(dt), f[iy1, ix].astype(dt), f[iy1, ix1].astype(dt))
        top = v00 * bx + v01 * ax
        bot = v10 * bx + v11 * ax
        s = top * by + bot * ay
    assert s.dtype == dt
    return s


def invert_flow_ref(f, max_iter, tol):
    """(out (H, W, 2) float32, residual (H, W) float32, not_converged, steps (H, W) int32 taken per pixel)."""
    assert f.dtype == F32 and f.ndim == 3 and f.shape[2] == 2 and max_iter >= 1
    H, W = f.shape[:2]
    tol = F32(tol)
    n = H * W
    qx = np.tile(np.arange(W, dtype=F32), H)
    qy = np.repeat(np.arange(H, dtype=F32), W)
    g = np.zeros((n, 2), F32)
    res = np.zeros(n, F32)
    steps = np.zeros(n, np.int32)
    live = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(max_iter):
            if live.size == 0:
                break
            gl = g[live]
            new = -sample(f, qx[live] - gl[:, 0], qy[live] - gl[:, 1], F32)
            d = np.abs(new - gl)
            g[live] = new
            res[live] = np.maximum(d[:, 0], d[:, 1])        # maximum propagates a NaN
            steps[live] += 1
            stop = (d[:, 0] <= tol) & (d[:, 1] <= tol)      # False for a NaN
            live = live[~stop]
    return g.reshape(H, W, 2), res.reshape(H, W), int(live.size), steps.reshape(H, W)


def _inside(px, py, H, W):
    with np.errstate(invalid="ignore"):
        return (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)


IDENTITY6 = np.array([1, 0, 0, 0, 1, 0], F64)


def to_moving_ref(pts, f, m6=None, pad=(0, 0)):
    """(out (n, 2) float64, converged (n,) uint8, inside (n,) uint8) of MA_POINTS_TO_MOVING."""
    assert pts.dtype == F64 and f.dtype == F32
    H, W = f.shape[:2]
    m = IDENTITY6 if m6 is None else np.asarray(m6, F64).ravel()
    ok = np.isfinite(pts).all(1)
    out = np.full(pts.shape, np.nan, F64)
    p = pts[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        u = p - sample(f, p[:, 0].copy(), p[:, 1].copy(), F64)
        ox = ((m[0] * u[:, 0] + m[1] * u[:, 1]) + m[2]) - F64(pad[0])
        oy = ((m[3] * u[:, 0] + m[4] * u[:, 1]) + m[5]) - F64(pad[1])
    out[ok] = np.stack([ox, oy], -1)
    inside = np.zeros(len(pts), np.uint8)
    inside[ok] = _inside(p[:, 0], p[:, 1], H, W)
    return out, ok.astype(np.uint8), inside


def to_reference_ref(pts, f, t6=None, pad=(0, 0), max_iter=50, tol=1e-4):
    """(out, converged, inside) of MA_POINTS_TO_REFERENCE, and the steps taken per point."""
    assert pts.dtype == F64 and f.dtype == F32 and max_iter >= 1
    H, W = f.shape[:2]
    t = IDENTITY6 if t6 is None else np.asarray(t6, F64).ravel()
    tol = F64(tol)
    ok = np.isfinite(pts).all(1)
    s = pts[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = s[:, 0] + F64(pad[0]), s[:, 1] + F64(pad[1])
        a = np.stack([(t[0] * sx + t[1] * sy) + t[2], (t[3] * sx + t[4] * sy) + t[5]], -1)
        p = a.copy()
        conv = np.zeros(len(s), np.uint8)
        steps = np.zeros(len(s), np.int32)
        live = np.arange(len(s))
        for _ in range(max_iter):
            if live.size == 0:
                break
            pl = p[live]
            new = a[live] + sample(f, pl[:, 0].copy(), pl[:, 1].copy(), F64)
            d = np.abs(new - pl)
            p[live] = new
            steps[live] += 1
            stop = (d[:, 0] <= tol) & (d[:, 1] <= tol)
            conv[live[stop]] = 1
            live = live[~stop]
    out = np.full(pts.shape, np.nan, F64)
    out[ok] = p
    converged = np.zeros(len(pts), np.uint8)
    converged[ok] = conv
    inside = np.zeros(len(pts), np.uint8)
    inside[ok] = _inside(p[:, 0], p[:, 1], H, W)
    all_steps = np.zeros(len(pts), np.int32)
    all_steps[ok] = steps
    return out, converged, inside, all_steps


# ---- the analytic test flows ------------------------------------------------------------------------------------------
# name -> (fx(x, y), fy(x, y), analytic Lipschitz constant La, analytic bilinear error constant E), float64 functions;
# per component La sums the maxima of |d/dx| and |d/dy| and E the maxima of |d2/dx2| and |d2/dy2| over 8; each is the
# larger of the two components'.  None where the flow folds (La > 1).
ANALYTIC = {
    "A": (lambda x, y: 3 * np.sin(x / 17) + 2 * np.cos(y / 23), lambda x, y: 2.5 * np.cos(x / 13 + y / 31),
          max(3 / 17 + 2 / 23, 2.5 / 13 + 2.5 / 31), max(3 / 17 ** 2 + 2 / 23 ** 2, 2.5 / 13 ** 2 + 2.5 / 31 ** 2) / 8),
    "B": (lambda x, y: 20 * np.sin(x / 90) * np.cos(y / 70) + 5, lambda x, y: 15 * np.cos(x / 110 + y / 80) - 3,
          max(20 / 90 + 20 / 70, 15 / 110 + 15 / 80), max(20 / 90 ** 2 + 20 / 70 ** 2, 15 / 110 ** 2 + 15 / 80 ** 2) / 8),
    "C": (lambda x, y: 6 * np.sin(x / 9), lambda x, y: 6 * np.cos(y / 9), 6 / 9, 6 / 9 ** 2 / 8),
    "F": (lambda x, y: 12 * np.sin(x / 9), lambda x, y: 0 * y, None, None),
}
SHAPE = (700, 900)


def analytic_flow(name, shape=SHAPE):
    H, W = shape
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    fx, fy = ANALYTIC[name][:2]
    return np.stack([fx(x, y), fy(x, y)], -1).astype(F32)


def lipschitz(f):
    """From the array: per component the maximum |adjacent difference| along x plus the maximum along y; the larger of
    the two components."""
    f = f.astype(F64)
    dx = np.abs(np.diff(f, axis=1)).reshape(-1, 2).max(0) if f.shape[1] > 1 else np.zeros(2)
    dy = np.abs(np.diff(f, axis=0)).reshape(-1, 2).max(0) if f.shape[0] > 1 else np.zeros(2)
    return float((dx + dy).max())


def analytic_inverse(name, shape=SHAPE, iters=400):
    """g*(q) = q - p* with p* - f(p*) = q solved in float64 on the analytic flow (a contraction: La < 1), and the mask of
    pixels whose p* lies inside the image."""
    H, W = shape
    fx, fy, La, _ = ANALYTIC[name]
    assert La is not None and La < 1
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    px, py = x.copy(), y.copy()
    for _ in range(iters):
        px, py = x + fx(px, py), y + fy(px, py)
    assert max(np.abs(px - (x + fx(px, py))).max(), np.abs(py - (y + fy(px, py))).max()) < 1e-11
    return np.stack([x - px, y - py], -1), _inside(px, py, H, W)
