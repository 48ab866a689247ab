"""Write tests/golden/cv2_remap_4.5.5.npz: OpenCV's own cv2.remap in its four interpolation modes.

    python tests/golden/make_cv2_remap_golden.py        # numpy + opencv-contrib-python==4.5.5.64, nothing else

Holds, for uint8, uint16 and float32 (BORDER_CONSTANT 0, the default):
  * cv2.remap(src, map, None, mode) for INTER_NEAREST / LINEAR / CUBIC / LANCZOS4 of seeded images (1 and 3 channels, one
    of them 2 x 3 px) over seeded maps: random subpixel, exact integers, half pixels, a smooth map that crosses every
    source edge (both of OpenCV's summation paths), and non-finite / huge coordinates; for float32 also an image with
    NaN and +-Inf pixels;
  * impulse images (one non-zero pixel in the middle of a 24 x 24 zero image) remapped at all 32 x 32 fractions with the
    impulse under every tap: entry (fy * k + k1, fx * k + k2) is the 2-D weight of tap (k1, k2) at fraction (fy, fx)
    times the impulse -- OpenCV's 2-D tables themselves (exactly for float32).
tests/test_cv2_remap_golden.py compares the CPU restatement (and, under -m gpu, the HIP path) with it."""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cv2_remap_4.5.5.npz")
MODES = {"nearest": 0, "linear": 1, "cubic": 2, "lanczos4": 4}
KOFF = {"linear": (2, 0), "cubic": (4, 1), "lanczos4": (8, 3)}   # taps per axis, offset of the first tap
DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
SRC_SHAPES = [(37, 45, 1), (19, 23, 3), (2, 3, 1)]
IMPULSE = {"u8": 255, "u16": 65535, "f32": 1.0}
IMP_SIDE, IMP_AT = 24, 12


def image(h, w, cn, dtype, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w) if cn == 1 else (h, w, cn)
    if dtype == np.float32:
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=dtype)


def nonfinite_image(seed):
    img = image(37, 45, 1, np.float32, seed)
    img[0, 0] = np.nan
    img[18, 20] = np.nan
    img[5, 40] = np.inf
    img[30, 3] = -np.inf
    img[36, 44] = -0.0
    return img


def maps(sh, sw, seed, dh=21, dw=27):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:dh, 0:dw].astype(np.float64)
    sub = np.stack([rng.uniform(-5, sw + 5, (dh, dw)), rng.uniform(-5, sh + 5, (dh, dw))], -1).astype(np.float32)
    integer = np.stack([rng.integers(-3, sw + 3, (dh, dw)), rng.integers(-3, sh + 3, (dh, dw))], -1).astype(np.float32)
    half = (integer + np.float32(0.5)).astype(np.float32)
    edges = np.stack([xx * ((sw + 12) / (dw - 1)) - 6 + 0.37, yy * ((sh + 12) / (dh - 1)) - 6 + 0.61], -1).astype(np.float32)
    bad = sub.copy()
    bad[0, 0] = (np.nan, 1.0)
    bad[1, 1] = (2.0, np.nan)
    bad[2, 2] = (np.inf, 3.0)
    bad[3, 3] = (-np.inf, -np.inf)
    bad[4, :4] = (1e12, -1e12)
    bad[5, :4] = (40000.0, 3.0)
    bad[6, :4] = (-40000.0, 2.5)
    return {"subpixel": sub, "integer": integer, "half": half, "edges": edges, "bad": bad}


def impulse_map(mode):
    """(32 k, 32 k, 2) map: entry (fy k + k1, fx k + k2) puts the impulse under tap (k1, k2) at fraction (fy, fx)"""
    k, off = KOFF[mode]
    fy, k1, fx, k2 = np.meshgrid(np.arange(32), np.arange(k), np.arange(32), np.arange(k), indexing="ij")
    mx = (IMP_AT + off - k2) + fx / 32.0
    my = (IMP_AT + off - k1) + fy / 32.0
    return np.stack([mx, my], -1).reshape(32 * k, 32 * k, 2).astype(np.float32)


def impulse_image(dt):
    img = np.zeros((IMP_SIDE, IMP_SIDE), DTYPES[dt])
    img[IMP_AT, IMP_AT] = IMPULSE[dt]
    return img


def main():
    import cv2
    assert cv2.__version__.startswith("4.5.5"), cv2.__version__
    out = {}
    for dn, dt in DTYPES.items():
        for si, (h, w, cn) in enumerate(SRC_SHAPES):
            src = image(h, w, cn, dt, 100 * si + len(dn))
            out[f"{dn}_s{si}_src"] = src
            for mn, m in maps(h, w, 7 * si + 1).items():
                out[f"{dn}_s{si}_{mn}_map"] = m
                for mode, code in MODES.items():
                    out[f"{dn}_s{si}_{mn}_{mode}"] = cv2.remap(src, m, None, code)
        for mode in KOFF:
            out[f"{dn}_impulse_{mode}"] = cv2.remap(impulse_image(dn), impulse_map(mode), None, MODES[mode])
    nf = nonfinite_image(5)
    out["nonfinite_src"] = nf
    for mn, m in maps(37, 45, 9).items():
        out[f"nonfinite_{mn}_map"] = m
        for mode, code in MODES.items():
            out[f"nonfinite_{mn}_{mode}"] = cv2.remap(nf, m, None, code)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays")


if __name__ == "__main__":
    main()
