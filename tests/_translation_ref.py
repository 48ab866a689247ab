"""The numpy statement of include/microaligner_translation.h: a plain loop over the shifts, one pair of slices and int64
sums per shift, Python integers for num / va / vb and float(int) for their conversion, the peak rule, and the level loop of
align_translation written over injected pyr_down and label functions.  Nothing of the product is used."""
import math

import numpy as np


def overlap(h, w, dx, dy):
    """(y0, y1, x0, x1) of O(d), or None when it is empty"""
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    return None if y1 <= y0 or x1 <= x0 else (y0, y1, x0, x1)


def moments(a, b, window):
    """(5, ny, nx) uint64: S_ab, S_a, S_aa, S_b, S_bb at every shift of window = (dx0, dx1, dy0, dy1); 0 where n = 0."""
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 2
    h, w = a.shape
    dx0, dx1, dy0, dy1 = window
    out = np.zeros((5, dy1 - dy0 + 1, dx1 - dx0 + 1), np.uint64)
    A, B = a.astype(np.int64), b.astype(np.int64)
    for dy in range(dy0, dy1 + 1):
        for dx in range(dx0, dx1 + 1):
            o = overlap(h, w, dx, dy)
            if o is None:
                continue
            y0, y1, x0, x1 = o
            pa, pb = A[y0:y1, x0:x1], B[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            out[:, dy - dy0, dx - dx0] = [(pa * pb).sum(dtype=np.int64), pa.sum(dtype=np.int64), (pa * pa).sum(dtype=np.int64),
                                          pb.sum(dtype=np.int64), (pb * pb).sum(dtype=np.int64)]
    return out


def count(h, w, dx, dy):
    return 0 if abs(dx) >= w or abs(dy) >= h else (h - abs(dy)) * (w - abs(dx))


def score(n, S_ab, S_a, S_aa, S_b, S_bb):
    """one score from Python integers: exact num, va, vb, each rounded once by float()"""
    n, S_ab, S_a, S_aa, S_b, S_bb = (int(v) for v in (n, S_ab, S_a, S_aa, S_b, S_bb))
    if n == 0:
        return math.nan
    num, va, vb = n * S_ab - S_a * S_b, n * S_aa - S_a * S_a, n * S_bb - S_b * S_b
    if va == 0 or vb == 0:
        return math.nan
    return float(num) / (math.sqrt(float(va)) * math.sqrt(float(vb)))


def scores(shape, window, mom):
    h, w = shape
    dx0, dx1, dy0, dy1 = window
    out = np.full(mom.shape[1:], np.nan)
    for j in range(out.shape[0]):
        for i in range(out.shape[1]):
            out[j, i] = score(count(h, w, dx0 + i, dy0 + j), *mom[:, j, i])
    return out


def peak(shape, window, table, exclude):
    """the dict Context.translation_search gives (without the table)"""
    dx0, dx1, dy0, dy1 = window
    ny, nx = table.shape
    best = None
    for j in range(ny):
        for i in range(nx):
            s = table[j, i]
            if np.isfinite(s):
                dx, dy = dx0 + i, dy0 + j
                key = (-s, dx * dx + dy * dy, dy, dx)
                if best is None or key < best:
                    best = key
    if best is None:
        return dict(dx=0, dy=0, delta_x=0.0, delta_y=0.0, score=math.nan, second=math.nan, n=0, at_limit=False, valid=False)
    dy, dx = best[2], best[3]
    j, i = dy - dy0, dx - dx0
    s0 = table[j, i]

    def refine(pos, length, sm, sp):
        if pos == 0 or pos == length - 1:
            return 0.0
        sm, sp = sm(), sp()
        if not (np.isfinite(sm) and np.isfinite(sp)):
            return 0.0
        den = sm - 2.0 * s0 + sp
        if not den < 0.0:
            return 0.0
        return float(min(max(0.5 * (sm - sp) / den, -0.5), 0.5))
    far = [table[jj, ii] for jj in range(ny) for ii in range(nx)
           if max(abs(jj - j), abs(ii - i)) > exclude and np.isfinite(table[jj, ii])]
    return dict(dx=dx, dy=dy, delta_x=refine(i, nx, lambda: table[j, i - 1], lambda: table[j, i + 1]),
                delta_y=refine(j, ny, lambda: table[j - 1, i], lambda: table[j + 1, i]), score=float(s0),
                second=float(max(far)) if far else math.nan, n=count(shape[0], shape[1], dx, dy),
                at_limit=bool(i == 0 or i == nx - 1 or j == 0 or j == ny - 1), valid=True)


def search(a, b, window, exclude):
    """-> (the dict of peak(), the table)"""
    table = scores(a.shape, window, moments(a, b, window))
    return peak(a.shape, window, table, exclude), table


def align_translation_ref(ref, mov, pyr_down, make_labels, max_shift=None, min_overlap=0.5, coarse_side=512, refine_radius=2,
                          finest_level=0, exclude=2, min_score=None):
    """The level loop of align_translation over pyr_down(img) and make_labels(img) -> u8.
    -> (tmat, dict(levels=[dict(level, shape, window, peak, score, second, n, at_limit)], shift, score, score0, distinct,
    at_limit, valid, accepted))."""
    refs, movs = [ref], [mov]
    while max(refs[-1].shape) > coarse_side and min((refs[-1].shape[0] + 1) // 2, (refs[-1].shape[1] + 1) // 2) >= 32:
        refs.append(pyr_down(refs[-1]))
        movs.append(pyr_down(movs[-1]))
    top = len(refs) - 1
    last = min(finest_level, top)
    info = dict(levels=[], shift=(0.0, 0.0), score=math.nan, score0=math.nan, distinct=math.nan, at_limit=False, valid=False,
                accepted=False)
    above = None
    for lv in range(top, last - 1, -1):
        h, w = refs[lv].shape
        lim = []
        for side in (w, h):
            v = int(math.floor((1.0 - min_overlap) * side))
            if max_shift is not None:
                v = min(v, int(math.ceil(max_shift / 2.0 ** lv)))
            lim.append(v)
        if above is None:
            window = (-lim[0], lim[0], -lim[1], lim[1])
        else:
            cx, cy = (min(max(2 * above[k], -lim[k]), lim[k]) for k in (0, 1))
            window = (max(-lim[0], cx - refine_radius), min(lim[0], cx + refine_radius),
                      max(-lim[1], cy - refine_radius), min(lim[1], cy + refine_radius))
        a, b = make_labels(refs[lv]), make_labels(movs[lv])
        res, table = search(a, b, window, exclude)
        info["levels"].append(dict(level=lv, shape=(h, w), window=window, peak=(res["dx"], res["dy"]), score=res["score"],
                                   second=res["second"], n=res["n"], at_limit=res["at_limit"]))
        if not res["valid"]:
            return np.eye(2, 3), info
        if lv == top:
            info["distinct"] = res["score"] - res["second"]
        info["at_limit"] = info["at_limit"] or res["at_limit"]
        above = (res["dx"], res["dy"])
    info["valid"] = True
    info["score"] = res["score"]
    if window[0] <= 0 <= window[1] and window[2] <= 0 <= window[3]:
        info["score0"] = float(table[-window[2], -window[0]])
    else:
        info["score0"] = search(a, b, (0, 0, 0, 0), exclude)[0]["score"]
    info["shift"] = (2.0 ** last * (res["dx"] + res["delta_x"]), 2.0 ** last * (res["dy"] + res["delta_y"]))
    info["accepted"] = bool((min_score is None or info["score"] >= min_score)
                            and (above == (0, 0) or info["score"] > info["score0"]))
    tmat = np.array([[1.0, 0.0, -info["shift"][0]], [0.0, 1.0, -info["shift"][1]]]) if info["accepted"] else np.eye(2, 3)
    return tmat, info
