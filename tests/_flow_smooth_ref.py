"""The numpy float32 statement of include/microaligner_flowsmooth.h: taps, the weighted smoothing in both modes with every
weight kind, the fold mask and the repair loop.  numpy rounds every float32 operation on its own and keeps denormals, which
is the arithmetic the header asks of the kernels, so the kernels must give these bits."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MAX_RADIUS, MAX_MARGIN = 128, 32


def gaussian_taps(sigma, truncate=3.0):
    """t[0 .. r]: r = max(1, ceil(truncate * sigma)), t_k = exp(-k^2 / (2 sigma^2)) in float64, divided by
    t_0 + 2 sum(t_k), then rounded to float32."""
    r = max(1, int(math.ceil(float(truncate) * float(sigma))))
    if r > MAX_RADIUS:
        raise ValueError(f"r = {r} > {MAX_RADIUS}")
    k = np.arange(r + 1, dtype=F64)
    t = np.exp(-k * k / (2.0 * float(sigma) ** 2))
    return (t / (t[0] + 2.0 * t[1:].sum())).astype(F32)


def pixel_weight(weight, shape, cell_size=None):
    """weight(p) as an (H, W) float32 map: None -> ones; uint8 -> nonzero = 1.0; float32 (H, W) as it is; with cell_size
    (cell_h, cell_w) a (gy, gx) float32 map on the grid from (0, 0), the last row and column ragged."""
    H, W = shape
    if weight is None:
        return np.ones((H, W), F32)
    if cell_size is not None:
        ch, cw = cell_size
        assert weight.dtype == F32 and weight.shape == (-(-H // ch), -(-W // cw))
        return np.ascontiguousarray(weight[(np.arange(H) // ch)[:, None], (np.arange(W) // cw)[None, :]])
    assert weight.shape == (H, W)
    if weight.dtype == np.uint8:
        return (weight != 0).astype(F32)
    assert weight.dtype == F32
    return weight


def fir(P, taps, axis):
    """the header's rule along `axis`, samples outside the array being 0"""
    P = np.moveaxis(np.asarray(P, F32), axis, -1)
    n = P.shape[-1]
    A = taps[0] * P
    for k in range(1, len(taps)):
        lo, hi = np.zeros_like(P), np.zeros_like(P)
        if k < n:
            lo[..., k:] = P[..., :n - k]      # P(x - k)
            hi[..., :n - k] = P[..., k:]      # P(x + k)
        A = A + taps[k] * (lo + hi)
    return np.moveaxis(A, -1, axis)


def effective_weight(flow, wmap):
    ok = np.isfinite(wmap) & (wmap > 0) & np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1])
    return np.where(ok, wmap, F32(0)).astype(F32)


def smooth_flow_ref(flow, taps, weight=None, cell_size=None, mode="all", min_support=0.0):
    """(out, unsupported) of the header's smoothing"""
    assert flow.dtype == F32 and taps.dtype == F32 and mode in ("all", "blend")
    H, W = flow.shape[:2]
    min_support = F32(min_support)
    with np.errstate(all="ignore"):
        w = effective_weight(flow, pixel_weight(weight, (H, W), cell_size))
        live = w > 0
        planes = [np.where(live, w * flow[..., 0], F32(0)), np.where(live, w * flow[..., 1], F32(0)), w]
        S0, S1, S2 = (fir(fir(p.astype(F32), taps, 1), taps, 0) for p in planes)
        good = S2 > min_support
        s = np.full((H, W, 2), np.nan, F32)
        s[..., 0][good] = (S0[good] / S2[good]).astype(F32)
        s[..., 1][good] = (S1[good] / S2[good]).astype(F32)
        unsupported = int((~good).sum())
        if mode == "all":
            return s, unsupported
        rs, cs = fir(np.ones(W, F32), taps, 0), fir(np.ones(H, F32), taps, 0)
        sn = cs[:, None] * rs[None, :]
        c = S2 / sn
        d = F32(4) * c - F32(2)
        a = np.where(d > 0, np.where(d < 1, d, F32(1)), F32(0)).astype(F32)
        mixed = s + a[..., None] * (flow - s)
        out = np.where((live & (a == 1))[..., None], flow, np.where(live[..., None], mixed, s)).astype(F32)
    return out, unsupported


def det_j(flow):
    """det J of microaligner_qc.h: float64, numpy.gradient derivatives (0 along an axis of length 1)"""
    u, v = flow[..., 0].astype(F64), flow[..., 1].astype(F64)
    H, W = u.shape
    with np.errstate(all="ignore"):
        gx = (lambda a: np.gradient(a, axis=1)) if W > 1 else np.zeros_like
        gy = (lambda a: np.gradient(a, axis=0)) if H > 1 else np.zeros_like
        return (1.0 + gx(u)) * (1.0 + gy(v)) - gy(u) * gx(v)


def fold_mask_ref(flow, margin):
    """(keep uint8, (folded, invalid, dropped))"""
    det = det_j(flow)
    with np.errstate(all="ignore"):
        folded = np.isfinite(det) & (det <= 0)
    invalid = ~(np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1]))
    bad = folded | invalid
    H, W = bad.shape
    pad = np.zeros((H + 2 * margin, W + 2 * margin), bool)
    pad[margin:margin + H, margin:margin + W] = bad
    along_x = np.zeros((H + 2 * margin, W), bool)
    for d in range(2 * margin + 1):
        along_x |= pad[:, d:d + W]
    hit = np.zeros((H, W), bool)
    for d in range(2 * margin + 1):
        hit |= along_x[d:d + H]
    return (~hit).astype(np.uint8), (int(folded.sum()), int(invalid.sum()), int(hit.sum()))


def repair_flow_ref(flow, sigma=6.0, margin=4, max_rounds=8):
    """(flow, rounds, converged, flows after each smoothing round): the loop of repair_flow()"""
    taps = gaussian_taps(sigma)
    rounds, steps, converged = [], [], False
    for _ in range(max_rounds):
        keep, (folded, invalid, dropped) = fold_mask_ref(flow, margin)
        if folded == 0 and invalid == 0:
            converged = True
            break
        flow, unsupported = smooth_flow_ref(flow, taps, keep, None, "blend", 0.0)
        rounds.append((folded, invalid, dropped, unsupported))
        steps.append(flow)
    else:
        _, (folded, invalid, _) = fold_mask_ref(flow, margin)
        converged = folded == 0 and invalid == 0
    return flow, rounds, converged, steps


def repair_case():
    """the 96 x 160 field of the repair tests: smooth, three folding bumps, two NaN holes, an inf corner, a NaN edge run"""
    H, W = 96, 160
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    u = 3 * np.sin(x / 17) + 2 * np.cos(y / 23)
    v = 2.5 * np.cos(x / 13 + y / 31)
    for x0, y0, s, A in ((40, 30, 5, 1.7), (120, 60, 4, 2.2), (3, 90, 3, 1.5)):
        g = np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * s ** 2))
        u -= A * (x - x0) * g
        v -= 0.5 * A * (y - y0) * g
    f = np.stack([u, v], -1)
    f[20:62, 58:100] = np.nan
    f[50:57, 80:91] = np.nan
    f[0, 0] = np.inf
    f[H - 1, W - 3:] = np.nan
    return f.astype(F32)
