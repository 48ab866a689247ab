"""The numpy statement of include/microaligner_quantile.h: the population, the order statistic by np.sort and the rank rule,
and the range normalisation in float32 with one array operation per rounding."""
import math

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)


def population(img, ignore_zeros=False):
    """(the population as a 1-D array, nonfinite, zeros): for float32, NaN and +-Inf are left out and -0.0 counts as +0.0;
    with ignore_zeros the zeros are left out as well."""
    v = np.asarray(img).ravel()
    nonfinite = zeros = 0
    if v.dtype == np.float32:
        finite = np.isfinite(v)
        nonfinite = int(v.size - finite.sum())
        v = v[finite] + np.float32(0.0)
    if ignore_zeros:
        keep = v != 0
        zeros = int(v.size - keep.sum())
        v = v[keep]
    return v, nonfinite, zeros


def image_quantiles(img, q, ignore_zeros=False):
    """(values float64, (pop, nonfinite, zeros)): element floor(q * (pop - 1)) of the sorted population; NaN when pop == 0."""
    v, nonfinite, zeros = population(img, ignore_zeros)
    pop = int(v.size)
    qs = np.atleast_1d(np.asarray(q, np.float64))
    if pop == 0:
        return np.full(qs.size, np.nan), (0, nonfinite, zeros)
    s = np.sort(v)
    ranks = [int(math.floor(float(x) * float(pop - 1))) for x in qs]
    return np.array([float(s[r]) for r in ranks], np.float64), (pop, nonfinite, zeros)


def normalize_range_u8(img, lo, hi):
    """v = float32(src) * float32(scale) + float32(shift), clamped to [0, 255] (NaN -> 0), rounded half to even."""
    lo, hi = float(lo), float(hi)
    d = hi - lo
    scale = 255.0 * (1.0 / d if d > DBL_EPSILON else 0.0)
    shift = 0.0 - lo * scale
    with np.errstate(all="ignore"):
        v = np.asarray(img).astype(np.float32) * np.float32(scale)
        v = v + np.float32(shift)
        v = np.fmin(np.fmax(v, np.float32(0.0)), np.float32(255.0))      # fmaxf / fminf: a NaN gives the other operand
        return np.rint(v).astype(np.uint8)


def normalize_percentile(img, low=0.0, high=99.9, ignore_zeros=False):
    """(u8 image, dict of lo, hi, pop, nonfinite, zeros, degenerate) with q = p / 100."""
    (lo, hi), (pop, nonfinite, zeros) = image_quantiles(img, [low / 100.0, high / 100.0], ignore_zeros)
    degenerate = pop == 0 or not hi > lo
    out = np.zeros(np.asarray(img).shape, np.uint8) if pop == 0 else normalize_range_u8(img, lo, hi)
    return out, dict(lo=float(lo), hi=float(hi), pop=pop, nonfinite=nonfinite, zeros=zeros, degenerate=degenerate)


def hot_pixel_image(seed=7, h=301, w=517):
    """A tissue-like uint16 image: background 200 + Poisson(30), a few hundred blurred nuclei up to ~2700, and ONE pixel at
    65535."""
    rng = np.random.default_rng(seed)
    img = 200.0 + rng.poisson(30, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(220):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2.5, 6.0)
        amp = rng.uniform(600, 2450)
        y0, y1, x0, x1 = max(0, int(cy - 4 * r)), min(h, int(cy + 4 * r) + 1), max(0, int(cx - 4 * r)), min(w, int(cx + 4 * r) + 1)
        g = amp * np.exp(-((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) / (2 * r * r))
        img[y0:y1, x0:x1] = np.maximum(img[y0:y1, x0:x1], 200.0 + g)
    img = np.clip(np.rint(img), 0, 65535).astype(np.uint16)
    img[h // 3, w // 2] = 65535
    return img
