"""ma_match_similarity (csrc/ransac.hip) restated in plain numpy and Python float64, with a trace of the path a call takes.

match_ref() is the reference of tests/test_gpu_match.py; tests/test_match_ref.py proves on the CPU that it equals the project's
definition (feature_reg/sparse_cpu.py:estimate_affine_partial_2d over the good matches) bit for bit and that its fit is the
least-squares solution.  Nothing here calls into sparse_cpu.

The statement follows the device's STRUCTURE where the structure can go wrong -- the compaction walks the queries in blocks of
1024 and places a block's good matches behind those of the blocks before it (`base`), the samples are scored in two instalments
([0, 256), then [256, max_iters), the second one only when the loop gets there) and a scored sample is `first + block` -- so
that a slip in one of these terms has a counterpart here to compare the cases against.

Numbers of csrc/ransac.hip restated as plain numbers: 1024 queries per compaction block (RS_F), 256 samples in the first
instalment (RS_FIRST), at most 10 re-selections.
"""
import math

import numpy as np

RS_F, RS_FIRST, REFINE_CAP = 1024, 256, 10
TWO_P24, TWO_P53 = 16777216.0, 9007199254740992.0


def ratio_path(nq, max_iters):
    """Which ratio kernels the device takes: a block per 1024 queries in two launches when there is more than one block and
    the blocks' counts fit the samples' count array (max_iters ints), else the single block that walks the queries."""
    nb = (nq + RS_F - 1) // RS_F
    return "two_launch" if 1 < nb <= max_iters else "single"


def ratio_good(idx, dist_sq, n_train, ratio):
    """The ratio test, entirely in float32: sqrt(d0) < ratio * sqrt(d1), and a first neighbour inside the train set."""
    d = np.asarray(dist_sq, np.float32).reshape(-1, 2)
    i0 = np.asarray(idx).reshape(-1, 2)[:, 0].astype(np.int64)
    with np.errstate(invalid="ignore"):
        r0, r1 = np.sqrt(d[:, 0]), np.sqrt(d[:, 1])
        assert r0.dtype == np.float32 and (np.float32(ratio) * r1).dtype == np.float32
        return (r0 < np.float32(ratio) * r1) & (i0 >= 0) & (i0 < n_train)


def compact(good, idx, qpts, tpts):
    """The point pairs of the good matches in the order of the queries, placed block by block as the kernels do: slot =
    good matches of the blocks before (`base`) + good matches before it in its block.  -> (n, sx, sy, dx, dy)."""
    nq = len(good)
    q32 = np.asarray(qpts, np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)
    t32 = np.asarray(tpts, np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)
    i0 = np.asarray(idx).reshape(-1, 2)[:, 0].astype(np.int64)
    out = np.full((4, nq), np.nan)
    base = 0
    for q0 in range(0, nq, RS_F):
        g = np.nonzero(good[q0:q0 + RS_F])[0] + q0
        slot = base + np.arange(len(g))
        out[0, slot], out[1, slot] = q32[g, 0], q32[g, 1]
        out[2, slot], out[3, slot] = t32[i0[g], 0], t32[i0[g], 1]
        base += len(g)
    return (base,) + tuple(np.ascontiguousarray(out[k, :base]) for k in range(4))


def residuals(m, sx, sy, dx, dy):
    """err = ex ex + ey ey with ex = ((a x - b y) + tx) - u, ey = ((b x + a y) + ty) - v, one rounding per operation."""
    a, b, tx, ty = m
    ex = ((a * sx - b * sy) + tx) - dx
    ey = ((b * sx + a * sy) + ty) - dy
    return ex * ex + ey * ey


def inliers(m, sx, sy, dx, dy, thr2):
    return residuals(m, sx, sy, dx, dy) < thr2


def two_point_model(sx, sy, dx, dy, i, j):
    """The similarity through the pairs i and j, or None for a degenerate sample."""
    xi, yi, xj, yj = float(sx[i]), float(sy[i]), float(sx[j]), float(sy[j])
    if abs(xi - xj) <= 1e-8 + 1e-5 * abs(xj) and abs(yi - yj) <= 1e-8 + 1e-5 * abs(yj):
        return None
    ux, uy, vx, vy = xj - xi, yj - yi, float(dx[j]) - float(dx[i]), float(dy[j]) - float(dy[i])
    den = ux * ux + uy * uy
    if den == 0.0:
        return None
    a = (vx * ux + vy * uy) / den
    b = (vy * ux - vx * uy) / den
    tx = float(dx[i]) - (a * xi - b * yi)
    ty = float(dy[i]) - (b * xi + a * yi)
    return a, b, tx, ty


def score_instalment(sx, sy, dx, dy, pairs, first, count, thr2, counts, on_thr):
    """rs_score_samples<<<count>>>(first): block k scores sample first + k; -1 for a degenerate sample.  on_thr (for the
    trace): pairs whose residual under the sample's model is EXACTLY thr^2 -- the strict comparison leaves them out."""
    for block in range(count):
        s = first + block
        m = two_point_model(sx, sy, dx, dy, pairs[s][0], pairs[s][1])
        if m is None:
            counts[s], on_thr[s] = -1, 0
            continue
        err = residuals(m, sx, sy, dx, dy)
        counts[s], on_thr[s] = int(np.count_nonzero(err < thr2)), int(np.count_nonzero(err == thr2))


def iterations(count, n, confidence, max_iters, it):
    w = count / n
    one = 1.0 - w * w
    denom = math.log(one if one > 1e-12 else 1e-12)
    if not denom < 0:
        return it
    need = math.ceil(math.log(1.0 - confidence) / denom)
    return need if need < max_iters else max_iters


def fit(sx, sy, dx, dy, mask, means=None):
    """Closed-form least squares over the masked pairs from integer sums about the centre floor(mean); the sums are taken in
    Python integers (the device's parallel sums of integers below 2^53 are as exact).  None: rank deficient."""
    n = int(np.count_nonzero(mask))
    if n < 2:
        return None
    fn = float(n)
    x, y, u, v = ([int(t) for t in c[mask]] for c in (sx, sy, dx, dy))
    mean = [float(sum(c)) / fn for c in (x, y, u, v)]
    if means is not None:
        means[:] = mean
    cx, cy, cu, cv = (float(math.floor(t)) for t in mean)
    x, y, u, v = ([t - int(c) for t in col] for col, c in ((x, cx), (y, cy), (u, cu), (v, cv)))
    Sx, Sy, Su, Sv = float(sum(x)), float(sum(y)), float(sum(u)), float(sum(v))
    Sxx = float(sum(p * p + q * q for p, q in zip(x, y)))
    Sxu = float(sum(p * r + q * t for p, q, r, t in zip(x, y, u, v)))
    Sxv = float(sum(p * t - q * r for p, q, r, t in zip(x, y, u, v)))
    D = fn * Sxx - (Sx * Sx + Sy * Sy)
    if not D > 0.0:
        return None
    a = (fn * Sxu - (Sx * Su + Sy * Sv)) / D
    b = (fn * Sxv - (Sx * Sv - Sy * Su)) / D
    tx = (Su - (a * Sx - b * Sy)) / fn
    ty = (Sv - (b * Sx + a * Sy)) / fn
    tx = (tx + cu) - (a * cx - b * cy)
    ty = (ty + cv) - (b * cx + a * cy)
    return a, b, tx, ty


def match_ref(idx, dist_sq, qpts, tpts, n_train, ratio=0.5, confidence=0.99, thr=3.0, max_iters=2000, seed=0):
    """-> (matrix (2, 3) float64 | None, n_good, status, trace).  status: 0 matrix valid, 1 fewer than 3 good matches,
    2 no model, 3 not computed (coordinates the exact sums do not cover).

    trace: ratio_path "single" | "two_launch"; n_good, status; exit "too_few" | "not_integer" | "magnitude" | "no_model" |
    "first_fit_failed" | "ok"; good (bool per query); and, once RANSAC runs: samples (consumed), instalments (1 or 2),
    degenerate (among the consumed), winner (sample index), winner_count, boundary (residuals of EXACTLY thr^2 met by the
    consumed samples), rounds (refits after a changed re-selection; 10: the cap ended the loop), mask (final
    inliers), means (the four means of the last fit, before floor), pairs (the compacted sx, sy, dx, dy)."""
    idx = np.asarray(idx).reshape(-1, 2)
    nq = len(idx)
    good = ratio_good(idx, dist_sq, n_train, ratio)
    n, sx, sy, dx, dy = compact(good, idx, qpts, tpts)
    trace = {"ratio_path": ratio_path(nq, max_iters), "good": good, "n_good": n}

    def done(mat, status, exit_):
        trace["status"], trace["exit"] = status, exit_
        return mat, n, status, trace
    if n < 3:
        return done(None, 1, "too_few")
    c = np.stack([sx, sy, dx, dy])
    ok = (c == np.floor(c)) & (np.abs(c) < TWO_P24)
    if not ok.all():
        return done(None, 3, "not_integer")
    cmax = float(int(np.abs(c).max()))
    if float(n) * 8.0 * cmax * cmax >= TWO_P53:
        return done(None, 3, "magnitude")

    thr2 = thr * thr
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = [tuple(int(t) for t in rng.choice(n, 2, replace=False)) for _ in range(max_iters)]
    counts, on_thr = [None] * max_iters, [0] * max_iters
    best, best_count, iters, it, scored, instalments, degenerate = -1, 0, max_iters, 0, 0, 0, 0
    while it < iters:
        if it >= scored:
            upto = min(RS_FIRST, max_iters) if scored == 0 else max_iters
            score_instalment(sx, sy, dx, dy, pairs, scored, upto - scored, thr2, counts, on_thr)
            scored = upto
            instalments += 1
        cnt = counts[it]
        it += 1
        if cnt < 0:
            degenerate += 1
            continue
        if cnt > best_count:
            best_count, best = cnt, it - 1
            iters = iterations(cnt, n, confidence, max_iters, it)
    trace.update(samples=it, instalments=instalments, degenerate=degenerate, winner=best, winner_count=best_count,
                 boundary=sum(on_thr[:it]))
    if best < 0 or best_count < 2:
        return done(None, 2, "no_model")

    m = two_point_model(sx, sy, dx, dy, pairs[best][0], pairs[best][1])
    best_mask = inliers(m, sx, sy, dx, dy, thr2)
    means = [0.0] * 4
    M = fit(sx, sy, dx, dy, best_mask, means)
    if M is None:
        return done(None, 2, "first_fit_failed")
    rounds = 0
    for _ in range(REFINE_CAP):
        mask = inliers(M, sx, sy, dx, dy, thr2)
        if np.count_nonzero(mask) < 2 or np.array_equal(mask, best_mask):
            break
        best_mask = mask
        M2 = fit(sx, sy, dx, dy, best_mask, means)
        if M2 is None:
            break
        M = M2
        rounds += 1
    trace.update(rounds=rounds, mask=best_mask, means=list(means), pairs=(sx, sy, dx, dy))
    a, b, tx, ty = M
    return done(np.array([[a, -b, tx], [b, a, ty]], np.float64), 0, "ok")
