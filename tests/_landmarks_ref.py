"""The numpy statement of include/microaligner_landmarks.h: the thin-plate-spline fit of landmark pairs, and its evaluation
with the header's terms formed in float64 exactly as the kernels form them and summed without rounding by math.fsum.
Independent of the package: it imports nothing from microaligner_amd."""
import math

import numpy as np


def tps_u(q):
    """U(q) = (0.5 * q) * log(q), U(0) = 0"""
    q = np.asarray(q, np.float64)
    out = np.zeros_like(q)
    pos = q > 0
    out[pos] = (0.5 * q[pos]) * np.log(q[pos])
    return out


def grid_nodes(n, s):
    return 1 if n == 1 else -(-(n - 1) // s) + 1


def fit(ref_pts, mov_pts, smoothing=0.0):
    """The header's fit, steps 1 without the refusals: a dict with the normalised centres u (n, 2), the weights w (n, 2), the
    affine part a (2, 3), c (2,), k, lam = smoothing * k^2 and the kernel matrix K."""
    r, m = np.asarray(ref_pts, np.float64), np.asarray(mov_pts, np.float64)
    n = r.shape[0]
    c = r.mean(axis=0)
    k = 1.0 / math.sqrt(np.mean(np.sum((r - c) ** 2, axis=1)))
    u = (r - c) * k
    d = u[:, None, :] - u[None, :, :]
    K = tps_u(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    lam = smoothing * k * k
    P = np.concatenate([u, np.ones((n, 1))], axis=1)
    A = np.block([[K + lam * np.eye(n), P], [P.T, np.zeros((3, 3))]])
    sol = np.linalg.solve(A, np.concatenate([m, np.zeros((3, 2))]))
    return dict(u=u, w=sol[:n], a=np.ascontiguousarray(sol[n:].T), c=c, k=k, lam=lam, K=K)


def records(f):
    """(cw (n, 4), a6 (6,)) of a fit(): what the kernels are fed"""
    return np.ascontiguousarray(np.concatenate([f["u"], f["w"]], axis=1)), np.ascontiguousarray(f["a"].ravel())


def evaluate(cw, a6, c, k, pts):
    """s (N, 2) at the float64 positions pts (N, 2): the n + 3 terms of each component as the header forms them, summed by
    math.fsum and rounded once.  Also mag (N, 2) = sum_i |w_i U_i| + |a_0 X| + |a_1 Y| + |a_2| per component, the scale of the
    derived error bound (n + 8) * 2^-53 * mag of a float64 evaluation in any order."""
    cw, a6, pts = np.asarray(cw, np.float64).reshape(-1, 4), np.asarray(a6, np.float64), np.asarray(pts, np.float64)
    X, Y = (pts[:, 0] - c[0]) * k, (pts[:, 1] - c[1]) * k
    d, e = X[:, None] - cw[None, :, 0], Y[:, None] - cw[None, :, 1]
    U = tps_u(d * d + e * e)
    s, mag = np.empty((pts.shape[0], 2)), np.empty((pts.shape[0], 2))
    for comp in range(2):
        terms = np.concatenate([cw[None, :, 2 + comp] * U, (a6[3 * comp] * X)[:, None], (a6[3 * comp + 1] * Y)[:, None],
                                np.full((pts.shape[0], 1), a6[3 * comp + 2])], axis=1)
        s[:, comp] = [math.fsum(row) for row in terms.tolist()]
        mag[:, comp] = np.abs(terms).sum(axis=1)
    return s, mag


def bound(mag, n):
    """the derived bound of the header's float64 evaluation against evaluate(): (n + 8) * 2^-53 * mag"""
    return (n + 8) * 2.0 ** -53 * mag


def node_positions(H, W, stride):
    """(gh * gw, 2) float64 pixel positions (x, y) of the nodes of the grid of an (H, W) flow at `stride`, row-major"""
    ys = np.minimum(np.arange(grid_nodes(H, stride), dtype=np.int64) * stride, H - 1)
    xs = np.minimum(np.arange(grid_nodes(W, stride), dtype=np.int64) * stride, W - 1)
    gx, gy = np.meshgrid(xs, ys)
    return np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float64)


def flow(cw, a6, c, k, H, W, stride=1):
    """(flow float64 (gh, gw, 2) = p - s(p) at the node positions, before the rounding to float32; bound of s (gh, gw, 2))"""
    p = node_positions(H, W, stride)
    s, mag = evaluate(cw, a6, c, k, p)
    shape = (grid_nodes(H, stride), grid_nodes(W, stride), 2)
    return (p - s).reshape(shape), bound(mag, np.asarray(cw).reshape(-1, 4).shape[0]).reshape(shape)
