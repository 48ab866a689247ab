"""The numpy statement of include/microaligner_flowaffine.h, written from its definitions: the per-pixel terms and counts of
the moments, summed per cell with math.fsum (the correctly rounded sum, which no order of summation reaches exactly but
every order approaches within the standard bound); apply(flow, A); and a fit that does not go through the moments at all:
numpy.linalg.lstsq over the pixels for the affine model and a direct minimisation over the parameters for the restricted
ones.  numpy rounds every float64 operation on its own, which is the arithmetic the header asks of the kernels."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MODELS = ("affine", "similarity", "rigid", "translation")


def pixel_weight(weight, shape, cell_size=None):
    """weight(p) as an (H, W) float32 map, by the kind of `weight`: None -> ones; (H, W) uint8 -> nonzero = 1.0; (H, W)
    float32 as it is; else a (gy, gx) float32 map on the cell grid of cell_size"""
    H, W = shape
    if weight is None:
        return np.ones((H, W), F32)
    if weight.shape == (H, W) and weight.dtype == np.uint8:
        return (weight != 0).astype(F32)
    if weight.shape == (H, W) and weight.dtype == F32:
        return weight
    ch, cw = cell_size
    assert weight.dtype == F32 and weight.shape == (-(-H // ch), -(-W // cw))
    return np.ascontiguousarray(weight[(np.arange(H) // ch)[:, None], (np.arange(W) // cw)[None, :]])


def pixel_terms(flow, weight=None, cell_size=None, prior=None, clip=None):
    """(terms (H, W, 14) float64, cls (H, W) int: 0 used, 1 invalid, 2 unweighted, 3 trimmed) of section 1; the terms of
    pixels that are not used are 0"""
    H, W = flow.shape[:2]
    wm = pixel_weight(weight, (H, W), cell_size)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    X = np.broadcast_to((np.arange(W, dtype=F64) - cx)[None, :], (H, W))
    Y = np.broadcast_to((np.arange(H, dtype=F64) - cy)[:, None], (H, W))
    u, v = flow[..., 0].astype(F64), flow[..., 1].astype(F64)
    finite = np.isfinite(u) & np.isfinite(v)
    weighted = np.isfinite(wm) & (wm > 0)
    cls = np.where(~finite, 1, np.where(~weighted, 2, 0))
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = X - u, Y - v
        if prior is not None:
            t = np.asarray(prior, F64).reshape(2, 3)
            rx = X - ((t[0, 0] * a + t[0, 1] * b) + t[0, 2])
            ry = Y - ((t[1, 0] * a + t[1, 1] * b) + t[1, 2])
            inside = (np.abs(rx) <= clip) & (np.abs(ry) <= clip)
            cls = np.where((cls == 0) & ~inside, 3, cls)
        w = wm.astype(F64)
        wa, wb = w * a, w * b
        terms = np.stack([w, wa, wb, wa * a, wa * b, wb * b, w * X, w * Y, wa * X, wb * X, wa * Y, wb * Y,
                          (w * u) * u, (w * v) * v], -1)
    terms[cls != 0] = 0.0
    return terms, cls


def cell_slices(shape, cell_size):
    H, W = shape
    ch, cw = (H, W) if cell_size is None else cell_size
    ch, cw = min(ch, H), min(cw, W)
    return [[(slice(y, min(y + ch, H)), slice(x, min(x + cw, W))) for x in range(0, W, cw)] for y in range(0, H, ch)]


def moments_ref(flow, weight=None, cell_size=None, prior=None, clip=None):
    """(sums (gy, gx, 14) by math.fsum, counts (gy, gx, 4) of used / invalid / unweighted / trimmed,
    abs_sums (gy, gx, 14) = sum |term|) per cell of cell_size (None: one cell)"""
    terms, cls = pixel_terms(flow, weight, cell_size, prior, clip)
    cells = cell_slices(flow.shape[:2], cell_size)
    gy, gx = len(cells), len(cells[0])
    sums, abs_sums, counts = np.zeros((gy, gx, 14)), np.zeros((gy, gx, 14)), np.zeros((gy, gx, 4), np.int64)
    for i in range(gy):
        for j in range(gx):
            t = terms[cells[i][j]].reshape(-1, 14)
            c = cls[cells[i][j]].ravel()
            t = t[c == 0]
            for k in range(14):
                sums[i, j, k] = math.fsum(t[:, k])
                abs_sums[i, j, k] = math.fsum(np.abs(t[:, k]))
            counts[i, j] = [(c == q).sum() for q in range(4)]
    return sums, counts, abs_sums


def apply_ref(flow, A):
    """apply(flow, A) of section 2"""
    A = np.asarray(A, F64).reshape(2, 3)
    H, W = flow.shape[:2]
    x = np.broadcast_to(np.arange(W, dtype=F64)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F64)[:, None], (H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = x - flow[..., 0].astype(F64), y - flow[..., 1].astype(F64)
        rx = (A[0, 0] * qx + A[0, 1] * qy) + A[0, 2]
        ry = (A[1, 0] * qx + A[1, 1] * qy) + A[1, 2]
        return np.stack([(x - rx).astype(F32), (y - ry).astype(F32)], -1)


def inverse(tmat):
    return np.linalg.inv(np.append(np.asarray(tmat, F64).reshape(2, 3), [[0, 0, 1]], axis=0))[:2]


def _used(flow, weight, cell_size):
    """(s (N, 2) centred sampling positions, p (N, 2) centred pixels, w (N,)) of the used pixels, and the centre"""
    H, W = flow.shape[:2]
    wm = pixel_weight(weight, (H, W), cell_size).astype(F64)
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    p = np.stack([x - c[0], y - c[1]], -1)
    f = flow.astype(F64)
    ok = np.isfinite(f).all(-1) & np.isfinite(wm) & (wm > 0)
    return (p - f)[ok], p[ok], wm[ok], c


def _absolute(L, t, c):
    return np.concatenate([L, (c + t - L @ c)[:, None]], 1)


def fit_ref(flow, model="affine", weight=None, cell_size=None):
    """The fit of the header without its moments, in absolute pixel coordinates.  "affine": numpy.linalg.lstsq on the rows
    sqrt(w) (s, 1) against sqrt(w) p.  The restricted models: the translation is eliminated through the weighted means
    (the optimum for any fixed L), and the linear part is found by minimising the cost over its parameters directly --
    "similarity": a linear least-squares problem in (alpha, beta), solved by lstsq on its own design matrix; "rigid": a
    Newton iteration on the angle, started from a coarse scan of the cost; "translation": L = I."""
    s, p, w, c = _used(flow, weight, cell_size)
    rw = np.sqrt(w)
    if model == "affine":
        A = np.concatenate([s, np.ones((len(s), 1))], 1) * rw[:, None]
        sol = np.linalg.lstsq(A, p * rw[:, None], rcond=None)[0]      # (3, 2)
        return _absolute(sol[:2].T, sol[2], c)
    ms, mp = (w[:, None] * s).sum(0) / w.sum(), (w[:, None] * p).sum(0) / w.sum()
    s0, p0 = s - ms, p - mp
    if model == "translation":
        L = np.eye(2)
    elif model == "similarity":
        # p0 ~ alpha (sx, sy) + beta (-sy, sx): rows for the x and the y equation of every pixel
        D = np.concatenate([np.stack([s0[:, 0], -s0[:, 1]], 1), np.stack([s0[:, 1], s0[:, 0]], 1)]) * np.tile(rw, 2)[:, None]
        al, be = np.linalg.lstsq(D, np.concatenate([p0[:, 0], p0[:, 1]]) * np.tile(rw, 2), rcond=None)[0]
        L = np.array([[al, -be], [be, al]])
    else:
        def cost_d(th):        # first and second derivative of sum w |p0 - R(th) s0|^2 by th
            cs, sn = math.cos(th), math.sin(th)
            Rs = np.stack([cs * s0[:, 0] - sn * s0[:, 1], sn * s0[:, 0] + cs * s0[:, 1]], 1)
            dRs = np.stack([-Rs[:, 1], Rs[:, 0]], 1)
            g = -2.0 * (w * ((p0 - Rs) * dRs).sum(1)).sum()
            h = 2.0 * (w * (p0 * Rs).sum(1)).sum()
            return g, h

        def cost(th):
            cs, sn = math.cos(th), math.sin(th)
            Rs = np.stack([cs * s0[:, 0] - sn * s0[:, 1], sn * s0[:, 0] + cs * s0[:, 1]], 1)
            return (w * ((p0 - Rs) ** 2).sum(1)).sum()
        scan = np.linspace(-math.pi, math.pi, 721)
        th = float(scan[int(np.argmin([cost(t) for t in scan]))])
        for _ in range(50):
            g, h = cost_d(th)
            if h <= 0:
                break
            step = g / h
            th -= step
            if abs(step) < 1e-17:
                break
        L = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    return _absolute(L, mp - L @ ms, c)


def weighted_rms(flow, tmat=None, weight=None, cell_size=None):
    """sqrt(sum w |f|^2 / sum w) over the used pixels; with tmat, of the residual p - tmat (s, 1) in float64"""
    s, p, w, c = _used(flow, weight, cell_size)
    if tmat is None:
        r = p - s
    else:
        t = np.asarray(tmat, F64)
        r = (p + c) - ((s + c) @ t[:, :2].T + t[:, 2])
    return math.sqrt((w * (r ** 2).sum(1)).sum() / w.sum())


def affine_flow(shape, inv_tmat):
    """the flow F(p) = p - M (p, 1) of the pure matrix registration whose inverse matrix M is `inv_tmat`: exact in float32
    when M is dyadic and the image small"""
    H, W = shape
    M = np.asarray(inv_tmat, F64).reshape(2, 3)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    sx = M[0, 0] * x + M[0, 1] * y + M[0, 2]
    sy = M[1, 0] * x + M[1, 1] * y + M[1, 2]
    f = np.stack([x - sx, y - sy], -1)
    assert np.array_equal(f.astype(F32).astype(F64), f), "the flow is not exact in float32"
    return f.astype(F32)


DYADIC_AFFINE = np.array([[1 + 2.0 ** -6, -2.0 ** -5, 3.5], [2.0 ** -5, 1 - 2.0 ** -7, -1.25]])
DYADIC_SIMILARITY = np.array([[1 + 2.0 ** -6, -2.0 ** -5, 3.5], [2.0 ** -5, 1 + 2.0 ** -6, -1.25]])


def bumpy_flow(shape=(97, 161), seed=7):
    """a 3 degree / 1 % similarity about the image centre plus a smooth field of about 0.3 px RMS"""
    H, W = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    th, sc = math.radians(3.0), 1.01
    L = sc * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    t = c - L @ c + np.array([2.25, -1.5])
    sx = L[0, 0] * x + L[0, 1] * y + t[0]
    sy = L[1, 0] * x + L[1, 1] * y + t[1]
    ph = rng.uniform(0, 2 * math.pi, 4)
    bx = 0.424 * np.sin(x / 19 + ph[0]) * np.cos(y / 23 + ph[1])
    by = 0.424 * np.cos(x / 17 + ph[2]) * np.sin(y / 29 + ph[3])
    return np.stack([x - sx + bx, y - sy + by], -1).astype(F32)
