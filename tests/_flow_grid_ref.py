"""CPU statements of include/microaligner_flowgrid.h in numpy, one array operation per rounding, written from the
definition there: the axis, sample, expand (float32), the loss maps, the float64 point sampler with the two point
transforms on it, and an independent float64 expansion (np.interp, separable).  TEST INFRASTRUCTURE, not product code."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24      # unit roundoff of float32

# Rounding of the float32 expansion against exact arithmetic on the same nodes, M = max |node|, first order in U:
#   stage x (top and bot alike): tx = fl(a / b) is off by at most U tx <= U, which moves the combination by at most
#   U |n01 - n00| <= 2 U M; bx = fl(1 - tx) is off by at most U / 2, times |n00| <= M: U M / 2 (taken as U M); the two
#   products round by at most U (|n00| bx + |n01| tx) <= U M; the sum by at most U M: 5 U M.
#   stage y: the same five terms on |top|, |bot| <= M, 5 U M, plus the convex combination of the two stage-x errors, 5 U M.
# 10 U M in all -- not the 8 a count of "three rounded stages" gives: each stage has the rounded weight pair on top of
# its two products and its sum.
EXPAND_ROUNDING = 10 * U * (1 + 1e-6)


def grid_nodes(n, s):
    return 1 if n == 1 else -(-(n - 1) // s) + 1


def node_positions(n, s):
    return np.minimum(np.arange(grid_nodes(n, s), dtype=np.int64) * s, n - 1)


def axis(n, s):
    """per pixel of the axis: (index of the cell's first node, of its second node, float32 weight of the second)"""
    x = np.arange(n, dtype=np.int64)
    g = grid_nodes(n, s)
    if g == 1:
        return np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, F32)
    P = node_positions(n, s)
    i = np.minimum(x // s, g - 2)
    t = (x - P[i]).astype(F32) / (P[i + 1] - P[i]).astype(F32)
    assert t.dtype == F32
    return i, i + 1, t


def sample_ref(flow, s):
    H, W = flow.shape[:2]
    return np.ascontiguousarray(flow[node_positions(H, s)][:, node_positions(W, s)])


def expand_ref(nodes, shape, s, rows=slice(None), cols=slice(None)):
    """E on the whole (H, W) grid, or on the crop rows x cols of it (slices)"""
    H, W = shape
    assert nodes.dtype == F32 and nodes.shape == (grid_nodes(H, s), grid_nodes(W, s), 2)
    j0, j1, ty = (a[rows] for a in axis(H, s))
    i0, i1, tx = (a[cols] for a in axis(W, s))
    tx, ty = tx[None, :, None], ty[:, None, None]
    n00, n01, n10, n11 = nodes[j0][:, i0], nodes[j0][:, i1], nodes[j1][:, i0], nodes[j1][:, i1]
    with np.errstate(invalid="ignore", over="ignore"):
        bx, by = F32(1) - tx, F32(1) - ty
        top = n00 * bx + n01 * tx
        bot = n10 * bx + n11 * tx
        e = top * by + bot * ty
    assert e.dtype == F32 and e.shape == (len(ty), tx.shape[1], 2)
    return e


def error_maps_ref(flow, nodes, s, cell, tol):
    """(max_err float32, above int64, invalid int64), each (gy, gx); cell = (cell_h, cell_w)"""
    H, W = flow.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        d = expand_ref(nodes, (H, W), s) - flow
    invalid = np.isnan(d).any(-1)
    e = np.maximum(np.abs(d[..., 0]), np.abs(d[..., 1]))
    assert e.dtype == F32
    ch, cw = min(cell[0], H), min(cell[1], W)
    gy, gx = -(-H // ch), -(-W // cw)
    max_err, above, inv = np.empty((gy, gx), F32), np.empty((gy, gx), np.int64), np.empty((gy, gx), np.int64)
    for cy in range(gy):
        for cx in range(gx):
            sl = (slice(cy * ch, min((cy + 1) * ch, H)), slice(cx * cw, min((cx + 1) * cw, W)))
            v = e[sl][~invalid[sl]]
            max_err[cy, cx] = v.max() if v.size else np.nan
            above[cy, cx] = int((v > F32(tol)).sum())
            inv[cy, cx] = int(invalid[sl].sum())
    return max_err, above, inv


def expand_f64(nodes, shape, s):
    """Independent of expand_ref: np.interp along x for every node row, then along y for every column, in float64."""
    H, W = shape
    Px, Py = node_positions(W, s).astype(F64), node_positions(H, s).astype(F64)
    n = nodes.astype(F64)
    rows = np.empty((n.shape[0], W, 2))
    for c in range(2):
        for j in range(n.shape[0]):
            rows[j, :, c] = np.interp(np.arange(W, dtype=F64), Px, n[j, :, c])
    out = np.empty((H, W, 2))
    for c in range(2):
        for x in range(W):
            out[:, x, c] = np.interp(np.arange(H, dtype=F64), Py, rows[:, x, c])
    return out


# ---- points -------------------------------------------------------------------------------------------------------------
def _axis64(c, n, s):
    g = grid_nodes(n, s)
    if g == 1:
        z = np.zeros(len(c), np.int64)
        return z, z, np.zeros(len(c), F64)
    P = node_positions(n, s)
    i = np.minimum(np.floor(c).astype(np.int64) // s, g - 2)
    t = (c - P[i].astype(F64)) / (P[i + 1] - P[i]).astype(F64)
    return i, i + 1, t


def sample_points_ref(nodes, shape, s, mx, my):
    """G64(mx, my) for 1-D float64 coordinate arrays: (n, 2) float64"""
    H, W = shape
    assert mx.dtype == F64 and my.dtype == F64
    with np.errstate(invalid="ignore", over="ignore"):
        cx = np.fmin(np.fmax(mx, F64(0)), F64(W - 1))
        cy = np.fmin(np.fmax(my, F64(0)), F64(H - 1))
        i0, i1, tx = _axis64(cx, W, s)
        j0, j1, ty = _axis64(cy, H, s)
        tx, ty = tx[:, None], ty[:, None]
        bx, by = F64(1) - tx, F64(1) - ty
        n00, n01, n10, n11 = (nodes[j0, i0].astype(F64), nodes[j0, i1].astype(F64), nodes[j1, i0].astype(F64),
                              nodes[j1, i1].astype(F64))
        top = n00 * bx + n01 * tx
        bot = n10 * bx + n11 * tx
        return top * by + bot * ty


def _inside(px, py, H, W):
    with np.errstate(invalid="ignore"):
        return (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)


IDENTITY6 = np.array([1, 0, 0, 0, 1, 0], F64)


def to_moving_grid_ref(pts, nodes, shape, s, m6=None, pad=(0, 0)):
    """(out, converged, inside) of MA_POINTS_TO_MOVING with G64 in place of S64"""
    H, W = shape
    m = IDENTITY6 if m6 is None else np.asarray(m6, F64).ravel()
    ok = np.isfinite(pts).all(1)
    out = np.full(pts.shape, np.nan, F64)
    p = pts[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        u = p - sample_points_ref(nodes, shape, s, p[:, 0].copy(), p[:, 1].copy())
        ox = ((m[0] * u[:, 0] + m[1] * u[:, 1]) + m[2]) - F64(pad[0])
        oy = ((m[3] * u[:, 0] + m[4] * u[:, 1]) + m[5]) - F64(pad[1])
    out[ok] = np.stack([ox, oy], -1)
    inside = np.zeros(len(pts), np.uint8)
    inside[ok] = _inside(p[:, 0], p[:, 1], H, W)
    return out, ok.astype(np.uint8), inside


def to_reference_grid_ref(pts, nodes, shape, s, t6=None, pad=(0, 0), max_iter=50, tol=1e-4):
    """(out, converged, inside) of MA_POINTS_TO_REFERENCE with G64 in place of S64"""
    H, W = shape
    t = IDENTITY6 if t6 is None else np.asarray(t6, F64).ravel()
    tol = F64(tol)
    ok = np.isfinite(pts).all(1)
    src = pts[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = src[:, 0] + F64(pad[0]), src[:, 1] + F64(pad[1])
        a = np.stack([(t[0] * sx + t[1] * sy) + t[2], (t[3] * sx + t[4] * sy) + t[5]], -1)
        p = a.copy()
        conv = np.zeros(len(src), np.uint8)
        live = np.arange(len(src))
        for _ in range(max_iter):
            if live.size == 0:
                break
            pl = p[live]
            new = a[live] + sample_points_ref(nodes, shape, s, pl[:, 0].copy(), pl[:, 1].copy())
            d = np.abs(new - pl)
            p[live] = new
            stop = (d[:, 0] <= tol) & (d[:, 1] <= tol)
            conv[live[stop]] = 1
            live = live[~stop]
    out = np.full(pts.shape, np.nan, F64)
    out[ok] = p
    converged = np.zeros(len(pts), np.uint8)
    converged[ok] = conv
    inside = np.zeros(len(pts), np.uint8)
    inside[ok] = _inside(p[:, 0], p[:, 1], H, W)
    return out, converged, inside


# ---- seeded inputs the CPU and GPU tests share ------------------------------------------------------------------------
def smooth_flow(shape, seed, amp=6.0):
    """a smooth flow of a few pixels: two sines per component with seeded phases and periods"""
    H, W = shape
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    px, py, qx, qy = r.uniform(20, 90, 4)
    ph = r.uniform(0, 6.28, 4)
    fx = amp * np.sin(x / px + ph[0]) * np.cos(y / py + ph[1]) + 0.5
    fy = 0.7 * amp * np.cos(x / qx + ph[2]) + 0.3 * amp * np.sin(y / qy + ph[3]) - 0.25
    return np.stack([fx, fy], -1).astype(F32)


def poison(a, seed, count=5):
    """a copy with NaN, +Inf, -Inf and 1e30 written at seeded places (count of each)"""
    a = a.copy()
    r = np.random.default_rng(seed)
    flat = a.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, 1e30):
        flat[r.integers(0, flat.size, min(count, flat.size))] = v
    return a
