"""The numpy float32 statement of include/microaligner_localcorr.h: the six products, the two smoothing passes, the score,
the weight, the classes and the per-cell counts.  numpy rounds every float32 operation on its own and keeps denormals, which
is the arithmetic the header asks of the kernels, so the kernels must give these bits (the sign and payload of a NaN apart).
Beside it a float64 statement of the same formula over scipy.ndimage.correlate1d, against which the float32 one is measured,
and the pair of images of the tests."""
import numpy as np

from _flow_smooth_ref import fir, pixel_weight

F32, F64 = np.float32, np.float64
AGREE, DISAGREE, FLAT, UNSUPPORTED = 0, 1, 2, 3
CLASSES = 4


def products(ref, img, center=(0.0, 0.0), weight=None):
    """(P0 .. P5) = (w, w A, w B, w A A, w B B, w A B) of the live pixels, zeros elsewhere"""
    assert img.dtype == F32 and img.shape == ref.shape
    with np.errstate(all="ignore"):
        A = np.asarray(ref).astype(F32) - F32(center[0])
        B = img - F32(center[1])
        w = pixel_weight(weight, ref.shape)
        live = np.isfinite(w) & (w > 0) & np.isfinite(A) & np.isfinite(B)
        wa, wb = w * A, w * B
        planes = (w, wa, wb, wa * A, wb * B, wa * B)
        return tuple(np.where(live, p, F32(0)).astype(F32) for p in planes)


def sums(ref, img, taps, center=(0.0, 0.0), weight=None):
    """(Sw, Sa, Sb, Saa, Sbb, Sab)"""
    assert taps.dtype == F32
    with np.errstate(all="ignore"):
        return tuple(fir(fir(p, taps, 1), taps, 0) for p in products(ref, img, center, weight))


def score_of(S, floor, min_support=0.0):
    """(s, va, vb) of the header; all three NaN where the window has no support"""
    Sw, Sa, Sb, Saa, Sbb, Sab = S
    floor, min_support = F32(floor), F32(min_support)
    with np.errstate(all="ignore"):
        ma, mb = Sa / Sw, Sb / Sw
        va = Saa / Sw - ma * ma
        vb = Sbb / Sw - mb * mb
        va = np.where(va < 0, F32(0), va)
        vb = np.where(vb < 0, F32(0), vb)
        c = Sab / Sw - ma * mb
        den = np.sqrt(va + floor) * np.sqrt(vb + floor)
        s = c / den
        s = np.where(s > 1, F32(1), np.where(s < -1, F32(-1), s))
        good = Sw > min_support
        nan = F32(np.nan)
        return tuple(np.where(good, v, nan).astype(F32) for v in (s, va, vb))


def weight_of(s, lo, hi):
    lo, hi = F32(lo), F32(hi)
    span = hi - lo
    with np.errstate(all="ignore"):
        return np.where(np.isnan(s) | (s < lo), F32(0), np.where(s >= hi, F32(1), (s - lo) / span)).astype(F32)


def classes(s, va, vb, floor, hi):
    """(H, W) uint8 of AGREE / DISAGREE / FLAT / UNSUPPORTED, tested in the header's order"""
    floor, hi = F32(floor), F32(hi)
    with np.errstate(all="ignore"):
        flat = (va <= floor) & (vb <= floor)
        return np.where(np.isnan(s), UNSUPPORTED, np.where(flat, FLAT, np.where(s >= hi, AGREE, DISAGREE))).astype(np.uint8)


def cell_counts(cls, cell_size, n=CLASSES):
    """_texture_ref.cell_counts for n classes: (gy, gx, n) int64 on the grid of cell_h x cell_w cells from (0, 0), the last
    row and column ragged"""
    H, W = cls.shape
    ch, cw = min(cell_size[0], H), min(cell_size[1], W)
    gy, gx = -(-H // ch), -(-W // cw)
    out = np.zeros((gy, gx, n), np.int64)
    cell = (np.arange(H) // ch)[:, None] * gx + (np.arange(W) // cw)[None, :]
    for k in range(n):
        out[..., k] = np.bincount(cell[cls == k], minlength=gy * gx).reshape(gy, gx)
    return out


def local_correlation_ref(ref, img, taps, floor, center=(0.0, 0.0), weight=None, lo=0.25, hi=0.75, min_support=0.0,
                          cell_size=None):
    """dict of score, weight, classes, va, vb and, with cell_size, counts"""
    s, va, vb = score_of(sums(ref, img, taps, center, weight), floor, min_support)
    out = {"score": s, "weight": weight_of(s, lo, hi), "classes": classes(s, va, vb, floor, hi), "va": va, "vb": vb}
    if cell_size is not None:
        out["counts"] = cell_counts(out["classes"], cell_size)
    return out


def local_correlation_f64(ref, img, taps, floor, center=(0.0, 0.0), weight=None, min_support=0.0):
    """The same formula in float64 over scipy.ndimage.correlate1d (zeros outside), from the same float32 inputs, taps and
    centres -> dict of score, Maa = Saa / Sw, Mbb = Sbb / Sw, va, vb (NaN where Sw <= min_support)."""
    from scipy.ndimage import correlate1d
    k = np.concatenate([taps[:0:-1], taps]).astype(F64)
    A = np.asarray(ref).astype(F32).astype(F64) - F64(F32(center[0]))
    B = img.astype(F64) - F64(F32(center[1]))
    w = pixel_weight(weight, ref.shape).astype(F64)
    live = np.isfinite(w) & (w > 0) & np.isfinite(A) & np.isfinite(B)
    w, A, B = np.where(live, w, 0.0), np.where(live, A, 0.0), np.where(live, B, 0.0)

    def smooth(p):
        return correlate1d(correlate1d(p, k, axis=1, mode="constant", cval=0.0), k, axis=0, mode="constant", cval=0.0)
    Sw, Sa, Sb, Saa, Sbb, Sab = (smooth(p) for p in (w, w * A, w * B, w * A * A, w * B * B, w * A * B))
    with np.errstate(all="ignore"):
        ma, mb = Sa / Sw, Sb / Sw
        Maa, Mbb = Saa / Sw, Sbb / Sw
        va, vb = np.maximum(Maa - ma * ma, 0.0), np.maximum(Mbb - mb * mb, 0.0)
        s = np.clip((Sab / Sw - ma * mb) / np.sqrt((va + floor) * (vb + floor)), -1.0, 1.0)
        good = Sw > min_support
        return {n: np.where(good, v, np.nan) for n, v in (("score", s), ("Maa", Maa), ("Mbb", Mbb), ("va", va), ("vb", vb))}


# ---- the pair of the tests -------------------------------------------------------------------------------------------------
NOISE = 0.004                        # of full scale, in both images
BLOCK = (slice(30, 50), slice(40, 70))      # 20 x 30, inside the texture
BLOCK_SHIFT = 7                      # along x: half a period of the texture's faster term


def full_scale(dtype):
    return {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}[np.dtype(dtype).type]


def values(H, W, dx=0.0, dy=0.0):
    """the pair's pattern in [0, 1] at (x + dx, y + dy): a texture, its right third constant 0.3"""
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    xs, ys = x + dx, y + dy
    v = 0.5 + 0.2 * np.cos(xs / 2.3) * np.cos(ys / 2.9) + 0.15 * np.cos(xs / 7 + ys / 5)
    return np.where(xs >= W - W // 3, 0.3, v)


def quantise(v, dtype):
    full = full_scale(dtype)
    v = v * full
    return v.astype(F32) if np.dtype(dtype) == F32 else np.clip(np.rint(v), 0, full).astype(dtype)


def pair(H, W, dtype, gain=0.8, bias=0.05, block=True, seed=3):
    """(ref of dtype, other image float32 in ref's grey levels, noise variance in squared grey levels): the other image is
    gain * v + bias with noise of its own, and with `block` a 20 x 30 block of it takes its content from 7 px away"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    v = values(H, W)
    o = v.copy()
    if block and H >= BLOCK[0].stop and W - W // 3 >= BLOCK[1].stop + BLOCK_SHIFT:
        o[BLOCK] = v[BLOCK[0], BLOCK[1].start + BLOCK_SHIFT:BLOCK[1].stop + BLOCK_SHIFT]
    n1, n2 = rng.normal(0, NOISE, (H, W)), rng.normal(0, NOISE, (H, W))
    full = full_scale(dtype)
    ref = quantise(v + n1, dtype)
    img = ((gain * o + bias + n2) * full).astype(F32)
    return ref, img, (NOISE * full) ** 2


def regions(H, W, margin):
    """masks of the cores of the texture (the block and its surroundings apart), the block and the constant part, `margin`
    px inside each"""
    tex, blk, flat = (np.zeros((H, W), bool) for _ in range(3))
    tex[margin:H - margin, margin:W - W // 3 - margin] = True
    tex[BLOCK[0].start - margin:BLOCK[0].stop + margin, BLOCK[1].start - margin:BLOCK[1].stop + margin] = False
    inner = min(margin, 6)
    blk[BLOCK[0].start + inner:BLOCK[0].stop - inner, BLOCK[1].start + inner:BLOCK[1].stop - inner] = True
    flat[margin:H - margin, W - W // 3 + margin:W - margin] = True
    return tex, blk, flat
