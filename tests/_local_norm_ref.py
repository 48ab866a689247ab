"""The numpy float32 statement of include/microaligner_localnorm.h: the live pixels, the two stages of smoothing, z, the two
outputs and the four counts.  numpy rounds every float32 operation on its own and keeps denormals, which is the arithmetic
the header asks of the kernels, so the kernels must give these bits.  Beside it a float64 twin of the same formula over
scipy.ndimage.correlate1d, against which the float32 one is measured, and the images of the tests."""
import numpy as np

from _flow_smooth_ref import fir, pixel_weight

F32, F64 = np.float32, np.float64
DROPPED, UNSUPPORTED, FLAT, CLIPPED = 0, 1, 2, 3
COUNTS = 4


def smooth(P, taps):
    """a row pass, then a column pass over its output"""
    return fir(fir(P, taps, 1), taps, 0)


def normalize_local_ref(img, taps, floor, clip=4.0, weight=None, min_support=0.0):
    """dict of z (NaN where the pixel has no z of its own), f32, u8 (None with an infinite clip), counts (4 ints), and
    the intermediates mu, Sw, v, live, supported"""
    assert taps.dtype == F32 and img.ndim == 2
    floor, clip, min_support = F32(floor), F32(clip), F32(min_support)
    zero = F32(0)
    with np.errstate(all="ignore"):
        x = np.asarray(img).astype(F32)
        w = pixel_weight(weight, img.shape)
        live = np.isfinite(w) & (w > 0) & np.isfinite(x)
        Sw = smooth(np.where(live, w, zero).astype(F32), taps)
        Sx = smooth(np.where(live, w * x, zero).astype(F32), taps)
        supported = Sw > min_support
        mu = Sx / Sw
        d = x - mu
        both = live & supported
        Sdd = smooth(np.where(both, (w * d) * d, zero).astype(F32), taps)
        v = Sdd / Sw
        z = (d / np.sqrt(v + floor)).astype(F32)
        has = both & ~np.isnan(z)
        f32 = np.where(has, np.minimum(np.maximum(z, -clip), clip), zero).astype(F32)
        u8 = None
        if np.isfinite(clip):
            scale = F32(127.0) / clip
            t = z * scale
            t = t + F32(128)
            t = np.fmin(np.fmax(t, zero), F32(255))          # fmax, fmin: a NaN sum takes the other operand
            u8 = np.where(has, np.rint(np.where(has, t, zero)), F32(128)).astype(np.uint8)
        counts = (int((~live).sum()), int((live & ~has).sum()), int((both & (v <= floor)).sum()),
                  int((both & (np.abs(z) > clip)).sum()))
    return {"z": np.where(has, z, F32(np.nan)).astype(F32), "f32": f32, "u8": u8, "counts": counts, "mu": mu, "Sw": Sw, "v": v,
            "live": live, "supported": supported}


def normalize_local_f64(img, taps, floor, clip=4.0, weight=None, min_support=0.0):
    """The same formula in float64 over scipy.ndimage.correlate1d (zeros outside), from the same inputs and float32 taps ->
    dict of z (NaN where the pixel has none), f32 (as float64), u8 (None with an infinite clip), v."""
    from scipy.ndimage import correlate1d
    k = np.concatenate([taps[:0:-1], taps]).astype(F64)
    floor, clip, min_support = F64(floor), F64(clip), F64(min_support)

    def smooth64(p):
        return correlate1d(correlate1d(p, k, axis=1, mode="constant", cval=0.0), k, axis=0, mode="constant", cval=0.0)
    with np.errstate(all="ignore"):
        x = np.asarray(img).astype(F64)
        w = pixel_weight(weight, img.shape).astype(F64)
        live = np.isfinite(w) & (w > 0) & np.isfinite(x)
        w, x = np.where(live, w, 0.0), np.where(live, x, 0.0)
        Sw, Sx = smooth64(w), smooth64(w * x)
        both = live & (Sw > min_support)
        mu = Sx / Sw
        d = np.where(both, x - mu, 0.0)
        v = smooth64(w * d * d) / Sw
        z = d / np.sqrt(v + floor)
        has = both & ~np.isnan(z)
        u8 = None
        if np.isfinite(clip):
            u8 = np.where(has, np.rint(np.clip(np.where(has, z, 0.0) * (127.0 / clip) + 128.0, 0.0, 255.0)), 128.0).astype(np.uint8)
        return {"z": np.where(has, z, np.nan), "f32": np.where(has, np.clip(z, -clip, clip), 0.0), "u8": u8, "v": v}


# ---- the images of the tests ------------------------------------------------------------------------------------------------
def full_scale(dtype):
    return {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}[np.dtype(dtype).type]


def floor_of(dtype):
    """on the data's scale: (0.01 of the dtype's range)^2"""
    return (0.01 * full_scale(dtype)) ** 2


def gain_field(H, W):
    """(g, o) of the usefulness table: a +-40 % gain and a +-30 grey level offset, both slow"""
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    g = 1 + 0.4 * np.sin(2 * np.pi * (1.5 * x / W + 0.2)) * np.cos(2 * np.pi * y / H)
    o = 30 * np.cos(2 * np.pi * (x / W + y / H))
    return g, o


def make_image(H, W, dtype, seed=0):
    """a texture and noise under a slow gain field over most of the dtype's range, its lower right corner exactly constant
    (flat windows), quantised to dtype"""
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    tex = 0.5 + 0.25 * np.cos(x / 2.3) * np.cos(y / 2.9) + 0.15 * np.cos(x / 7 + y / 5) + 0.05 * rng.normal(0, 1, (H, W))
    g = 0.6 + 0.35 * np.sin(2 * np.pi * (x / max(W, 2) + 0.1)) * np.cos(2 * np.pi * y / max(H, 2))
    v = np.clip(g * tex + 0.05, 0, 1)
    v[H - H // 4:, W - W // 4:] = 0.2
    full = full_scale(dtype)
    return (v * full).astype(F32) if np.dtype(dtype) == F32 else np.clip(np.rint(v * full), 0, full).astype(dtype)


def make_weight(H, W, seed=0):
    """a float32 weight with NaN, 0, negative and > 1 entries and (from 5 columns on) a band of zeros, and a uint8 mask
    with (from 5 rows on) a hole; in the middle of the band and of the hole a few lone live pixels, which a small window
    leaves without support"""
    rng = np.random.default_rng(77 * H + W + seed)
    w = rng.uniform(0.1, 2.5, (H, W)).astype(F32)
    pick = rng.random((H, W))
    w[pick < 0.04], w[(pick >= 0.04) & (pick < 0.08)], w[(pick >= 0.08) & (pick < 0.12)] = np.nan, 0.0, -1.0
    mask = (rng.random((H, W)) < 0.9).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
    if W >= 5:
        band = W // 5
        w[:, W // 3:W // 3 + band] = 0.0
        w[::5, W // 3 + band // 2] = 0.5
    if H >= 5:
        hole = H // 3
        mask[H // 4:H // 4 + hole] = 0
        mask[H // 4 + hole // 2, ::9] = 200
    return w, mask
