"""The numpy statement of the flat grey morphology (include/microaligner_morphology.h), shared by tests/test_morphology_ref.py
(no GPU), tests/test_gpu_morphology.py and the registry cases of tests/_gpu_cases/morphology.py.

It works on keys: the values themselves for uint8 and uint16, for float32 the signed key of the bits with every NaN turned
into the sentinel above (erosion) or below (dilation) every key, and the NaN of bits 0x7fc00000 where the sentinel is still
there at the end.  It is written plainly: the minimum over the window cut at the border, one shifted view per offset, along
x and then along y -- nothing of the kernel's blocks, halos or tiles."""
import numpy as np

OPS = ("erode", "dilate", "open", "close", "tophat", "blackhat")
DTYPES = (np.uint8, np.uint16, np.float32)
NAN_BITS = np.uint32(0x7fc00000)
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


def radii(radius):
    return (radius, radius) if isinstance(radius, (int, np.integer)) else tuple(radius)


def keys_of(img, maximum):
    """int64 keys of an image; a float32 NaN is the sentinel of the operation"""
    if img.dtype != np.float32:
        return img.astype(np.int64)
    bits = np.ascontiguousarray(img).view(np.int32)
    k = (bits ^ ((bits >> 31) & np.int32(0x7fffffff))).astype(np.int64)
    nan = (bits & np.int32(0x7fffffff)) > np.int32(0x7f800000)
    k[nan] = I32_MIN if maximum else I32_MAX
    return k


def values_of(keys, dtype, maximum):
    if np.dtype(dtype) != np.float32:
        return keys.astype(dtype)
    k = keys.astype(np.int32)
    bits = (k ^ ((k >> 31) & np.int32(0x7fffffff))).view(np.uint32)
    bits = np.where(keys == (I32_MIN if maximum else I32_MAX), NAN_BITS, bits)
    return bits.astype(np.uint32).view(np.float32)


def _along(keys, r, axis, maximum):
    """the minimum / maximum of keys over the cut window |d| <= r along one axis"""
    f = np.maximum if maximum else np.minimum
    out = keys.copy()
    n = keys.shape[axis]
    for d in range(1, min(r, n - 1) + 1):
        a = [slice(None)] * 2
        b = [slice(None)] * 2
        a[axis], b[axis] = slice(0, n - d), slice(d, n)
        a, b = tuple(a), tuple(b)
        out[a] = f(out[a], keys[b])          # the neighbour at +d
        out[b] = f(out[b], keys[a])          # the neighbour at -d
    return out


def primitive(img, radius, maximum):
    """ERODE (maximum=False) or DILATE of an image, in its dtype"""
    ry, rx = radii(radius)
    k = keys_of(img, maximum)
    k = _along(_along(k, rx, 1, maximum), ry, 0, maximum)
    return values_of(k, img.dtype, maximum)


def _minus(a, b):
    if a.dtype != np.float32:
        return (a.astype(np.int64) - b.astype(np.int64)).astype(a.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        d = a - b
    bits = d.view(np.uint32).copy()
    bits[np.isnan(d)] = NAN_BITS
    return bits.view(np.float32)


def morphology_ref(img, op, radius):
    """the statement of Context.morphology(img, op, radius)"""
    assert op in OPS and img.ndim == 2
    img = np.ascontiguousarray(img)
    if op == "erode":
        return primitive(img, radius, False)
    if op == "dilate":
        return primitive(img, radius, True)
    if op in ("open", "tophat"):
        o = primitive(primitive(img, radius, False), radius, True)
        return o if op == "open" else _minus(img, o)
    c = primitive(primitive(img, radius, True), radius, False)
    return c if op == "close" else _minus(c, img)


def all_ops_ref(img, radius):
    """{op: morphology_ref(img, op, radius)} for the six ops, each primitive computed once"""
    img = np.ascontiguousarray(img)
    e, d = primitive(img, radius, False), primitive(img, radius, True)
    o, c = primitive(e, radius, True), primitive(d, radius, False)
    return {"erode": e, "dilate": d, "open": o, "close": c, "tophat": _minus(img, o), "blackhat": _minus(c, img)}


def brute(img, radius, maximum):
    """ERODE / DILATE by a Python loop over every pixel and every pixel of its window"""
    ry, rx = radii(radius)
    H, W = img.shape
    k = keys_of(img, maximum)
    sent = I32_MIN if maximum else I32_MAX
    out = np.empty((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            best = sent
            for yy in range(max(0, y - ry), min(H, y + ry + 1)):
                for xx in range(max(0, x - rx), min(W, x + rx + 1)):
                    v = int(k[yy, xx])
                    best = max(best, v) if maximum else min(best, v)
            out[y, x] = best
    return values_of(out, img.dtype, maximum)


def bits(a):
    """what two results are compared by: float32 as uint32"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- inputs ---------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fa12345,     # NaNs
                     0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff,     # Inf, 0, denormals
                     0x7f7fffff, 0xff7fffff], np.uint32).view(np.float32)                                    # +-FLT_MAX


def make_image(h, w, dtype, seed=0, specials=True):
    """random values with smooth structure; float32 with NaNs of both signs, +-Inf, +-0, denormals and FLT_MAX sprinkled
    in and a block of NaNs larger than a small window"""
    rng = np.random.default_rng([seed, h, w, np.dtype(dtype).itemsize])
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.3 * np.sin(yy / 7.0) * np.cos(xx / 11.0) + 0.2 * rng.random((h, w))
    if np.dtype(dtype) == np.float32:
        img = ((base - 0.5) * 200.0).astype(np.float32)
        if specials:
            n = max(1, h * w // 16)
            img[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.choice(SPECIALS, n)
            img[h // 3:h // 3 + 9, w // 3:w // 3 + 12] = SPECIALS[rng.integers(0, 7, (min(9, h - h // 3), min(12, w - w // 3)))]
        return img
    top = np.iinfo(dtype).max
    img = np.clip(base * top, 0, top).astype(dtype)
    if specials:
        n = max(1, h * w // 16)
        img[rng.integers(0, h, n), rng.integers(0, w, n)] = rng.choice(np.array([0, top], dtype), n)
    return img
