"""The numpy statement of include/microaligner_flowmedian.h: keys, windows cut at the border, masks, the rank (n - 1) // 2,
the two modes, keep and the counts.  What the HIP kernels must give bit for bit."""
import numpy as np

F32 = np.float32
MAX_RADIUS = 7
_ABOVE = np.int64(1) << 40          # sorts behind every int32 key: a sample that is missing


def keys(a):
    """the order-preserving signed key of float32 bit patterns, int32"""
    b = np.ascontiguousarray(a, F32).view(np.int32)
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def values(k):
    """back from keys to float32: the map is its own inverse"""
    k = np.ascontiguousarray(k, np.int32)
    return (k ^ ((k >> 31) & np.int32(0x7fffffff))).view(F32)


def pixel_weight(weight, cell_size, H, W):
    """weight(q) of the header as an (H, W) float32 map"""
    if weight is None:
        return np.ones((H, W), F32)
    if cell_size is not None:
        ch, cw = (cell_size, cell_size) if isinstance(cell_size, int) else cell_size
        return np.asarray(weight, F32)[np.arange(H)[:, None] // ch, np.arange(W)[None, :] // cw]
    if weight.dtype == np.uint8:
        return (weight != 0).astype(F32)
    return np.asarray(weight, F32)


def participates(flow, weight=None, cell_size=None):
    H, W = flow.shape[:2]
    w = pixel_weight(weight, cell_size, H, W)
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0) & np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1])


def window_median(flow, r, weight=None, cell_size=None):
    """(m (H, W, 2) float32, part (H, W) bool, n (H, W) int): the lower median of the participating values of every
    window, NaN where n == 0"""
    assert flow.dtype == F32 and flow.ndim == 3 and flow.shape[2] == 2 and 1 <= r <= MAX_RADIUS
    H, W = flow.shape[:2]
    part = participates(flow, weight, cell_size)
    n = np.zeros((H, W), np.int64)
    pp = np.zeros((H + 2 * r, W + 2 * r), bool)
    pp[r:r + H, r:r + W] = part
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            n += pp[dy:dy + H, dx:dx + W]
    m = np.empty((H, W, 2), F32)
    rank = np.maximum(n - 1, 0) // 2
    for c in range(2):
        k = np.full((H + 2 * r, W + 2 * r), _ABOVE, np.int64)
        k[r:r + H, r:r + W] = np.where(part, keys(flow[..., c]).astype(np.int64), _ABOVE)
        stack = np.stack([k[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)])
        stack.sort(axis=0)
        sel = np.take_along_axis(stack, rank[None], 0)[0]
        m[..., c] = np.where(n > 0, values(np.where(n > 0, sel, 0).astype(np.int32)), F32(np.nan))
    return m, part, n


def finish(flow, m, part, n, where="all", thresh=np.inf):
    """(out, keep, (outliers, dropped, unsupported)) from the medians"""
    thresh = F32(thresh)
    assert thresh >= 0 and where in ("all", "outliers")
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.maximum(np.abs(flow[..., 0] - m[..., 0]), np.abs(flow[..., 1] - m[..., 1]))     # float32 operations
        outlier = part & (d > thresh)
    bad = outlier | ~part
    out = m.copy() if where == "all" else np.where(bad[..., None], m, flow)
    counts = (int(outlier.sum()), int((~part).sum()), int((n == 0).sum()))
    return out, (~bad).astype(np.uint8), counts


def median_flow_ref(flow, r=2, weight=None, cell_size=None, where="all", thresh=None):
    m, part, n = window_median(flow, r, weight, cell_size)
    return finish(flow, m, part, n, where, np.inf if thresh is None else thresh)


def spiked_flow(H=96, W=128, share=0.01, amp=20.0, seed=0, scale=1.0):
    """(clean, spiked, spikes, Lx, Ly): a smooth flow whose components change by at most Lx per pixel along x and Ly along y
    (measured on the float32 arrays), the same with +-amp px added to both components of about `share` of the pixels, and
    the mask of those pixels.  scale stretches the field: its slopes fall by that factor."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64) / scale
    clean = np.stack([3 * np.sin(x / 17) + 2 * np.cos(y / 23), 2.5 * np.cos(x / 13 + y / 31)], -1).astype(F32)
    spikes = rng.random((H, W)) < share
    sign = np.where(rng.random((H, W, 2)) < 0.5, -1.0, 1.0)
    spiked = np.where(spikes[..., None], clean.astype(np.float64) + amp * sign, clean).astype(F32)
    Lx = float(np.abs(np.diff(clean.astype(np.float64), axis=1)).max())
    Ly = float(np.abs(np.diff(clean.astype(np.float64), axis=0)).max())
    return clean, spiked, spikes, Lx, Ly


def window_count(mask, r):
    """the number of set pixels of `mask` in every window of radius r (cut at the border), and the windows' sizes"""
    H, W = mask.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    pad[r:r + H, r:r + W] = mask
    ones = np.zeros_like(pad)
    ones[r:r + H, r:r + W] = 1
    cnt, size = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            cnt += pad[dy:dy + H, dx:dx + W]
            size += ones[dy:dy + H, dx:dx + W]
    return cnt, size
