"""The numpy float32 statement of include/microaligner_texture.h: gradients, products, the two smoothing passes, the
eigenvalues, the weight, the classes and the per-cell counts.  numpy rounds every float32 operation on its own and keeps
denormals, which is the arithmetic the header asks of the kernels, so the kernels must give these bits (the sign and
payload of a NaN apart)."""
import numpy as np

from _flow_smooth_ref import fir

F32 = np.float32
TEXTURED, EDGE, FLAT = 0, 1, 2


def window_taps(winsize):
    """the solver's Gaussian window as taps t[0 .. r]: r = winsize // 2, sigma = 0.3 r, float64, normalised, then float32"""
    r = winsize // 2
    k = np.arange(r + 1, dtype=np.float64)
    t = np.exp(-k * k / (2.0 * (0.3 * r) ** 2))
    return (t / (t[0] + 2.0 * t[1:].sum())).astype(F32)


def products(img):
    """(P0, P1, P2) = (gx gx, gx gy, gy gy), central differences with a replicated border"""
    I = np.asarray(img).astype(F32)
    H, W = I.shape
    xs, ys = np.arange(W), np.arange(H)
    with np.errstate(all="ignore"):
        gx = F32(0.5) * (I[:, np.minimum(xs + 1, W - 1)] - I[:, np.maximum(xs - 1, 0)])
        gy = F32(0.5) * (I[np.minimum(ys + 1, H - 1), :] - I[np.maximum(ys - 1, 0), :])
        return gx * gx, gx * gy, gy * gy


def eigenvalues(img, taps):
    """(lam_min, lam_max) of the header"""
    assert taps.dtype == F32
    with np.errstate(all="ignore"):
        sxx, sxy, syy = (fir(fir(p, taps, 1), taps, 0) for p in products(img))
        h = F32(0.5) * (sxx + syy)
        d = F32(0.5) * (sxx - syy)
        q = np.sqrt(d * d + sxy * sxy)
        lam_max = h + q
        m = h - q
        lam_min = np.where(m < 0, F32(0), m)
    return lam_min.astype(F32), lam_max.astype(F32)


def weight_of(lam_min, floor):
    floor = F32(floor)
    with np.errstate(all="ignore"):
        live = lam_min > 0
        return np.where(live, lam_min / (lam_min + floor), F32(0)).astype(F32)


def classes(lam_min, lam_max, floor):
    """(H, W) uint8 of TEXTURED / EDGE / FLAT"""
    floor = F32(floor)
    with np.errstate(all="ignore"):
        textured = lam_min > floor
        edge = (lam_min <= floor) & (lam_max > floor)
    return np.where(textured, TEXTURED, np.where(edge, EDGE, FLAT)).astype(np.uint8)


def cell_counts(cls, cell_size):
    """(gy, gx, 3) int64 on the grid of cell_h x cell_w cells from (0, 0), the last row and column ragged"""
    H, W = cls.shape
    ch, cw = min(cell_size[0], H), min(cell_size[1], W)
    gy, gx = -(-H // ch), -(-W // cw)
    out = np.zeros((gy, gx, 3), np.int64)
    cell = (np.arange(H) // ch)[:, None] * gx + (np.arange(W) // cw)[None, :]
    for k in range(3):
        out[..., k] = np.bincount(cell[cls == k], minlength=gy * gx).reshape(gy, gx)
    return out


def texture_maps_ref(img, taps, floor=None, cell_size=None):
    """dict of lam_min, lam_max and, with floor, weight and classes, and, with cell_size, counts"""
    lam_min, lam_max = eigenvalues(img, taps)
    out = {"lam_min": lam_min, "lam_max": lam_max}
    if floor is not None:
        out["weight"] = weight_of(lam_min, floor)
        out["classes"] = classes(lam_min, lam_max, floor)
        if cell_size is not None:
            out["counts"] = cell_counts(out["classes"], cell_size)
    return out


def three_regions(dtype, H=96, W=160):
    """the 96 x 160 image of the statement's test: a cosine texture (columns [0, 56)), a constant part with a straight
    vertical edge at column 80 (columns [56, 104): a step of 0.4 of full scale), and a constant part (columns [104, 160)),
    all with noise of 0.4 % of full scale; -> (image, masks of the three regions' cores, full scale)"""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    v = np.full((H, W), 0.3)
    v[:, :56] = 0.5 + 0.2 * np.cos(x[:, :56] / 2.0) * np.cos(y[:, :56] / 2.5)
    v[:, 80:104] = 0.7
    v[:, 104:] = 0.5
    v += rng.normal(0, 0.004, (H, W))
    full = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}[dtype]
    img = v * full
    img = img.astype(F32) if dtype is np.float32 else np.clip(np.rint(img), 0, full).astype(dtype)
    core = np.zeros((3, H, W), bool)
    core[0, 16:-16, 8:40] = True        # texture
    core[1, 16:-16, 78:82] = True       # edge
    core[2, 16:-16, 124:152] = True     # flat
    return img, core, full
