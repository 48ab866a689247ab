"""The numpy statement of include/microaligner_flowfill.h: level 0 from the flow and the weight, the pull to 1 x 1, the top,
the push with kept pixels overriding, and the counts.  Vectorised per level; every operation is one numpy ufunc call, so
each is rounded on its own in `dtype`.  With dtype=float32 this is what the HIP kernels must give bit for bit; with
dtype=float64 the same formulas are the independent statement the float32 one is held to."""
import numpy as np

import _flow_smooth_ref as S

F32, F64 = np.float32, np.float64


def level0(flow, weight=None, cell_size=None, dtype=F32):
    """(a0 (H, W, 2), t0 (H, W)) in dtype: section 1 of the header.  The weight is read in float32, as the kernel does."""
    assert flow.dtype == F32 and flow.ndim == 3 and flow.shape[2] == 2
    H, W = flow.shape[:2]
    if isinstance(cell_size, int):
        cell_size = (cell_size, cell_size)
    w = S.pixel_weight(weight, (H, W), cell_size)
    with np.errstate(invalid="ignore"):
        kept = np.isfinite(w) & (w > 0) & np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1])
        t = np.where(kept, np.minimum(w, F32(1)), F32(0)).astype(dtype)
    a = np.where(kept[..., None], flow, F32(0)).astype(dtype)
    return a, t


def pull(a, t):
    """(a, t) of the parent level: section 2"""
    h, w = t.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    ap = np.zeros((2 * hc, 2 * wc, 2), a.dtype)
    tp = np.zeros((2 * hc, 2 * wc), t.dtype)
    ap[:h, :w] = a
    tp[:h, :w] = t
    c = [[(ap[dy::2, dx::2], tp[dy::2, dx::2]) for dx in (0, 1)] for dy in (0, 1)]
    with np.errstate(all="ignore"):
        sw = (c[0][0][1] + c[0][1][1]) + (c[1][0][1] + c[1][1][1])
        s = (c[0][0][1][..., None] * c[0][0][0] + c[0][1][1][..., None] * c[0][1][0]) + \
            (c[1][0][1][..., None] * c[1][0][0] + c[1][1][1][..., None] * c[1][1][0])
        has = sw > 0
        q = s / np.where(has, sw, 1).astype(sw.dtype)[..., None]
    return np.where(has[..., None], q, 0).astype(a.dtype), np.minimum(sw, 1).astype(t.dtype)


def _taps(n, nc, dtype):
    """(i0, i1, weight of i0, weight of i1) of the n pixels of a level along an axis whose parent has nc entries"""
    x = np.arange(n)
    even = x % 2 == 0
    i0 = np.where(even, x // 2 - 1, (x - 1) // 2)
    i1 = i0 + 1
    a = np.where(even, 0.25, 0.75).astype(dtype)
    b = np.where(even, 0.75, 0.25).astype(dtype)
    return np.clip(i0, 0, nc - 1), np.clip(i1, 0, nc - 1), a, b


def push(G, a, t):
    """G_l from G_{l+1} and (a_l, t_l): section 4"""
    h, w = t.shape
    hc, wc = G.shape[:2]
    assert (hc, wc) == ((h + 1) // 2, (w + 1) // 2)
    i0, i1, ax, bx = _taps(w, wc, a.dtype)
    j0, j1, ay, by = _taps(h, hc, a.dtype)
    with np.errstate(all="ignore"):
        rows = ax[None, :, None] * G[:, i0] + bx[None, :, None] * G[:, i1]
        up = ay[:, None, None] * rows[j0] + by[:, None, None] * rows[j1]
        mix = up + t[..., None] * (a - up)
    return np.where((t >= 1)[..., None], a, np.where((t == 0)[..., None], up, mix)).astype(a.dtype)


def fill_flow_ref(flow, weight=None, cell_size=None, dtype=F32):
    """(out in dtype, (dropped, blended, unsupported), levels)"""
    a, t = level0(flow, weight, cell_size, dtype)
    pyramid = [(a, t)]
    while pyramid[-1][1].shape != (1, 1):
        pyramid.append(pull(*pyramid[-1]))
    a, t = pyramid[-1]
    G = np.where((t > 0)[..., None], a, np.nan).astype(dtype)
    for a, t in pyramid[-2::-1]:
        G = push(G, a, t)
    t0 = pyramid[0][1]
    counts = (int((t0 == 0).sum()), int(((t0 > 0) & (t0 < 1)).sum()), int((~np.isfinite(G).all(-1)).sum()))
    return G, counts, len(pyramid) - 1


# ---- fields of the tests ---------------------------------------------------------------------------------------------------
def smooth_field(H, W, scale=1.0):
    """a smooth float32 flow of a few pixels"""
    y, x = np.mgrid[0:H, 0:W].astype(F64) / scale
    return np.stack([3 * np.sin(x / 17) + 2 * np.cos(y / 23), 2.5 * np.cos(x / 13 + y / 31)], -1).astype(F32)


def holed_case(H, W, seed=0):
    """(flow, weight float32) of the float32-against-float64 test: a smooth field; a rectangular hole half the image wide;
    20 % of the pixels dropped at random; 20 % of the pixels with soft weights in (0, 1)"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    f = smooth_field(H, W)
    w = np.ones((H, W), F32)
    r = rng.random((H, W))
    w[r < 0.2] = 0
    soft = (r >= 0.2) & (r < 0.4)
    w[soft] = rng.uniform(0.05, 0.95, (H, W)).astype(F32)[soft]
    w[H // 4:H // 4 + H // 3, W // 4:W // 4 + W // 2] = 0
    return f, w


def disc_case(n=512, diameter=150):
    """(flow, keep uint8, inside bool): a smooth n x n flow with a dropped disc in the middle"""
    f = smooth_field(n, n, scale=4.0)
    y, x = np.mgrid[0:n, 0:n]
    inside = (x - n // 2) ** 2 + (y - n // 2) ** 2 < (diameter / 2.0) ** 2
    return f, (~inside).astype(np.uint8), inside
