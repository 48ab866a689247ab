"""The matching step (csrc/ransac.hip: ratio test, ordered compaction, two-instalment sample scoring, refinement) on the paths
the random trials of test_feature_reg.py never reach: the cases, their expectations, and the checks (CPU only) that both are
right.  tests/test_gpu_match.py runs every case on the device and imports everything from here.

Every expectation is tests/_match_ref.py:match_ref, a restatement of the whole of ma_match_similarity in numpy and Python
float64 that returns a trace of the path taken.  This module proves, without a device,
  * that match_ref equals the project's definition (sparse_cpu.estimate_affine_partial_2d over the good matches) bit for bit,
  * that its final fit is the least-squares solution (exact rational arithmetic) and its final mask a fixed point,
  * that every case reaches the boundary it is named after: each carries a predicate over the trace, asserted below.
Parameters found by search (seeds, inlier shares, confidences) are written down as numbers; the predicates prove them.
"""
import functools
import os
import sys
import zlib
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _match_ref as MR  # noqa: E402
from microaligner_amd.feature_reg import sparse_cpu as SP  # noqa: E402

F32 = np.float32
N_CASES = 111            # the number of cases this module was written with


class Case:
    def __init__(self, name, idx, dist_sq, qpts, tpts, claim, n_train=None, ratio=0.5, confidence=0.99, thr=3.0,
                 max_iters=2000, seed=0, exact=None):
        self.name, self.claim, self.exact = name, claim, exact
        self.idx = np.ascontiguousarray(idx, np.int32)
        self.dist_sq = np.ascontiguousarray(dist_sq, F32)
        self.qpts, self.tpts = np.ascontiguousarray(qpts, np.float64), np.ascontiguousarray(tpts, np.float64)
        self.n_train = len(self.tpts) if n_train is None else n_train
        self.ratio, self.confidence, self.thr, self.max_iters, self.seed = ratio, confidence, thr, max_iters, seed
        assert self.idx.shape == self.dist_sq.shape == self.qpts.shape == (len(self.idx), 2) and self.tpts.shape[1] == 2
        assert len(self.idx) <= 3100 and max_iters <= 2000

    @property
    def params(self):
        return dict(ratio=self.ratio, confidence=self.confidence, thr=self.thr, max_iters=self.max_iters, seed=self.seed)

    def variant(self, name, claim, **kw):
        c = Case(name, self.idx, self.dist_sq, self.qpts, self.tpts, claim, n_train=self.n_train, **dict(self.params, **kw))
        return c


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = BY_NAME[name]
    return MR.match_ref(c.idx, c.dist_sq, c.qpts, c.tpts, c.n_train, **c.params)


def expected(case):
    """(matrix | None, n_good, status, trace) of a case, computed once per process and left unchanged."""
    return _expected(case.name)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- builders ------------------------------------------------------------------------------------------------------------
def embed(rng, src, dst, nq, good_at, ratio=0.5, lo=0, hi=1500, decoys=37):
    """A search result of nq queries in which exactly the queries `good_at` (ascending) pass the ratio test and carry the pairs
    (src[k], dst[k]) in that order; the others fail it and point at random train points.  The matched train points are
    scattered among decoys.  -> idx, dist_sq, qpts, tpts"""
    good_at = np.asarray(good_at, np.int64)
    assert len(good_at) == len(src) == len(dst) and (np.diff(good_at) > 0).all()
    qpts = rng.integers(lo, hi, (nq, 2)).astype(np.float64)
    nt = nq + decoys
    tpts = rng.integers(lo, hi, (nt, 2)).astype(np.float64)
    perm = rng.permutation(nt)[:nq]
    if len(good_at):
        qpts[good_at], tpts[perm[good_at]] = src, dst
    idx = np.stack([perm, rng.integers(0, nt, nq)], 1)
    r2 = float(F32(ratio)) ** 2
    d1 = rng.uniform(0.5, 2.0, nq).astype(F32)
    d0 = (d1 * r2 * rng.uniform(1.1, 3.0, nq)).astype(F32)
    d0[good_at] = (d1[good_at] * r2 * rng.uniform(0.05, 0.9, len(good_at))).astype(F32)
    return idx, np.stack([d0, d1], 1), qpts, tpts


def noisy_pairs(rng, n, share, sigma, lo=0, hi=1500):
    """n integer point pairs: a similarity plus noise, rounded to pixels; a pair is consistent with probability `share`."""
    th, sc = rng.uniform(-0.3, 0.3), rng.uniform(0.8, 1.25)
    A = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    src = rng.integers(lo, hi, (n, 2)).astype(np.float64)
    dst = src @ A.T + rng.integers(-40, 40, 2) + rng.normal(0, sigma, (n, 2))
    out = rng.random(n) >= share
    dst[out] = rng.integers(lo, hi, (int(out.sum()), 2))
    return src, np.rint(dst)


SHIFT = np.array([17.0, -9.0])
SHIFT_M = np.array([[1.0, 0.0, 17.0], [0.0, 1.0, -9.0]])


def compaction_cases(name, nq, good_at, claim, **kw):
    """Two cases over one pattern of good matches: `name`, whose good pairs are an exact integer translation (the matrix is
    known exactly; a pair taken from a wrong query or a wrong train point breaks it), and `name`_noisy, whose good pairs are a
    noisy similarity with outliers (the samples index the compacted list: a pair in the wrong slot changes the winner)."""
    good_at = np.asarray(good_at, np.int64)
    out = []
    for noisy in (False, True):
        nm = name + ("_noisy" if noisy else "")
        rng = _rng(nm)
        if noisy:
            src, dst = noisy_pairs(rng, len(good_at), 0.7, 1.2)
        else:
            src = rng.integers(0, 1500, (len(good_at), 2)).astype(np.float64)
            dst = src + SHIFT
        out.append(Case(nm, *embed(rng, src, dst, nq, good_at), claim,
                        exact=None if noisy or len(good_at) < 3 else SHIFT_M, **kw))
    return out


def sample_case(name, claim, n, share, sigma, data_seed=None, nq=None, lo=0, hi=1500, **kw):
    """n good matches of a noisy similarity (all queries good unless nq > n: then the good ones are a random subset)."""
    rng = _rng(name) if data_seed is None else np.random.default_rng(data_seed)
    src, dst = noisy_pairs(rng, n, share, sigma, lo, hi)
    nq = n if nq is None else nq
    good_at = np.sort(rng.permutation(nq)[:n])
    return Case(name, *embed(rng, src, dst, nq, good_at, lo=lo, hi=hi), claim, **kw)


def T(**want):
    """A predicate over the trace: every named entry equals the given value, or satisfies the given function."""
    def claim(trace):
        for k, v in want.items():
            got = trace.get(k)
            if not (v(got) if callable(v) else got == v):
                return False
        return True
    claim.want = want
    return claim


def _good_pattern_equals(mask):
    return lambda good: np.array_equal(good, mask)


CASES = []

# ---- compaction and ratio test -------------------------------------------------------------------------------------------
for _nq in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3100):
    _r = _rng("pattern%d" % _nq)
    _at = np.nonzero(_r.random(_nq) < 0.5)[0] if _nq > 3 else np.arange(_nq)
    CASES += compaction_cases("nq_%d" % _nq, _nq, _at, T(ratio_path="two_launch" if _nq >= 1025 else "single", n_good=len(_at),
                                                            status=0 if len(_at) >= 3 else 1))
_r = _rng("pattern_passes")
_at3100, _at2049 = np.nonzero(_r.random(3100) < 0.5)[0], np.nonzero(_r.random(2049) < 0.5)[0]
for _nq, _at, _mi, _path in ((3100, _at3100, 1, "single"), (3100, _at3100, 2, "single"), (3100, _at3100, 3, "single"),
                             (2049, _at2049, 2, "single"), (2049, _at2049, 3, "two_launch")):
    # (4 blocks against max_iters 1, 2, 3; 3 blocks against 2 and against 3: the counts array exactly full)
    CASES += compaction_cases("single_block_passes_nq%d_max_iters_%d" % (_nq, _mi), _nq, _at,
                              T(ratio_path=_path, n_good=len(_at), samples=lambda s, m=_mi: 1 <= s <= m), max_iters=_mi)
CASES += compaction_cases("two_launch_counts_exactly_full", 3100, _at3100, T(ratio_path="two_launch", n_good=len(_at3100)),
                          max_iters=4)
_at = _at3100[(_at3100 < 1024) | (_at3100 >= 2048)]
CASES += compaction_cases("empty_block", 3100, _at, T(ratio_path="two_launch", n_good=len(_at),
                                                      good=lambda g: g[:1024].any() and not g[1024:2048].any() and g[2048:].any()))
CASES += compaction_cases("empty_block_single", 3100, _at, T(ratio_path="single", n_good=len(_at)), max_iters=3)
for _name, _at in (("lane0_only", np.arange(0, 3100, 64)), ("lane63_only", np.arange(63, 3100, 64)),
                   ("last_query_only", np.array([5, 700, 1030, 3099])), ("first_of_each_block", np.arange(0, 3100, 1024)),
                   ("all_good", np.arange(3100)), ("none_good", np.arange(0))):
    CASES += compaction_cases(_name, 3100, _at, T(ratio_path="two_launch", n_good=len(_at), status=0 if len(_at) >= 3 else 1))
CASES += compaction_cases("last_query_alone", 3100, np.array([3099]), T(ratio_path="two_launch", n_good=1, status=1))
for _g in (0, 1, 2, 3):
    CASES += compaction_cases("n_good_%d" % _g, 200, np.array([7, 64, 199])[:_g],
                              T(n_good=_g, status=1 if _g < 3 else 0, exit="too_few" if _g < 3 else "ok"))


def _ratio_case(ratio):
    """Translation pairs on every query; the distances decide.  A third of the queries sit at d0 = 0.25 d1 and its two float32
    neighbours, a third at d0 = fl(ratio^2 d1) and up to two float32 steps either side, the rest are random.  What passes is
    numpy's float32 answer (match_ref); the case claims only that both outcomes occur among the boundary queries.  (These are
    the cases that need the correctly rounded float32 root on the device: with the 1 ulp hardware root the counts differed by
    up to 8 of 600.)"""
    name = "ratio_%s" % ratio
    rng = _rng(name)
    nq = 600
    src = rng.integers(0, 1500, (nq, 2)).astype(np.float64)
    idx, dist_sq, qpts, tpts = embed(rng, src, src + SHIFT, nq, np.arange(nq), ratio=ratio)
    d1 = dist_sq[:, 1]
    d0 = (d1 * rng.uniform(0.0, 1.2, nq)).astype(F32)
    k = np.arange(nq)
    quarter = d1 * F32(0.25)
    d0 = np.where(k % 9 == 0, quarter, d0)
    d0 = np.where(k % 9 == 1, np.nextafter(quarter, F32(0)), d0)
    d0 = np.where(k % 9 == 2, np.nextafter(quarter, F32(np.inf)), d0)
    edge = (F32(ratio) * F32(ratio)) * d1
    for j, steps in enumerate((-2, -1, 0, 1, 2)):
        e = edge.copy()
        for _ in range(abs(steps)):
            e = np.nextafter(e, F32(np.inf) if steps > 0 else F32(0))
        d0 = np.where(k % 9 == 3 + j, e, d0)
    dist_sq = np.stack([d0.astype(F32), d1], 1)
    at_edge = (k % 9 >= 3) & (k % 9 < 8)
    return Case(name, idx, dist_sq, qpts, tpts, T(status=0, good=lambda g: g[at_edge].any() and not g[at_edge].all()),
                ratio=ratio, exact=SHIFT_M)


CASES += [_ratio_case(r) for r in (0.5, 0.7, 0.8, 1.0)]


def _special_distances():
    """d0 = 0 < d1: good.  d0 = d1 = 0 (exact duplicates in the train set): 0 < 0 fails.  d1 = +Inf: good for any finite d0,
    and Inf < Inf fails.  NaN in either distance: every comparison with NaN fails."""
    name = "special_distances"
    rng = _rng(name)
    nq = 700
    src = rng.integers(0, 1500, (nq // 2, 2)).astype(np.float64)
    idx, dist_sq, qpts, tpts = embed(rng, src, src + SHIFT, nq, np.arange(0, nq, 2))
    good = np.zeros(nq, bool)
    good[0::2] = True
    for k, (d0, d1, ok) in enumerate(((0.0, 1.5, True), (0.0, 0.0, False), (3.0, np.inf, True), (np.inf, np.inf, False),
                                      (np.nan, 1.0, False), (0.1, np.nan, False), (np.nan, np.nan, False), (0.0, np.inf, True),
                                      (np.nan, np.inf, False), (0.0, np.nan, False))):
        for q in (10 + k, 64 * k + 63, nq - 1 - k):        # on a query that was good, on one that was not
            dist_sq[q] = d0, d1
            good[q] = ok
    return Case(name, idx, dist_sq, qpts, tpts, T(good=_good_pattern_equals(good), status=0))


CASES.append(_special_distances())

# ---- sample loop ---------------------------------------------------------------------------------------------------------
SECOND = sample_case("second_instalment", T(samples=lambda s: 256 < s < 2000, instalments=2, status=0), 600, 0.08, 1.2)
CASES.append(SECOND)
CASES.append(sample_case("winner_in_second_instalment", T(winner=lambda w: w >= 256, instalments=2, status=0), 600, 0.06, 1.2,
                         data_seed=0))
# (a second instalment that indexed its samples from 0 would still score [0, max_iters - 256) correctly: the winner has to lie
# behind that -- anywhere in a short second instalment, or in the last 256 samples of a full one)
CASES.append(sample_case("winner_in_short_second_instalment", T(winner=lambda w: 256 <= w < 512, instalments=2, status=0), 600, 0.06,
                         1.2, data_seed=7, max_iters=512))
CASES.append(sample_case("winner_in_the_last_256_samples", T(winner=lambda w: w >= 2000 - 256, instalments=2, status=0), 600, 0.06,
                         1.2, data_seed=11))
CASES.append(sample_case("exhausts_cap", T(samples=2000, instalments=2), 300, 0.0, 1.2))
# (the confidences: 1 - (1 - w^2)^(N - 1/2) for the share w of the best sample of the data, so that the count comes to N)
STOPS_DATA = dict(n=400, share=0.13, sigma=1.0, data_seed=12)      # best sample: 41 of 400, the 102nd
STOPS_CONFIDENCE = {255: 0.931982, 256: 0.932697, 257: 0.933404}
for _n in (255, 256, 257):
    CASES.append(sample_case("stops_at_%d" % _n, T(samples=_n, instalments=1 if _n <= 256 else 2, status=0),
                             confidence=STOPS_CONFIDENCE[_n], **STOPS_DATA))
for _mi in (1, 2, 255, 256, 257):
    CASES.append(SECOND.variant("max_iters_%d" % _mi, T(samples=_mi, instalments=2 if _mi > 256 else 1), max_iters=_mi))


def _coinciding(name, claim, which, **kw):
    rng = _rng(name)
    n = 300
    src, dst = noisy_pairs(rng, n, 0.2, 1.0)
    if which == "first_pair":      # the pair numpy draws first at this seed and this n
        i, j = np.random.Generator(np.random.PCG64(kw.get("seed", 0))).choice(n, 2, replace=False)
        src[j] = src[i]
    elif which == "all":
        src[:] = src[0]
    else:
        src[::2] = src[0]
    return Case(name, *embed(rng, src, dst, n, np.arange(n)), claim, **kw)


CASES.append(_coinciding("first_sample_degenerate_max_iters_1", T(status=2, exit="no_model", samples=1, degenerate=1, winner=-1),
                         "first_pair", max_iters=1))
CASES.append(_coinciding("all_sources_coincide", T(status=2, exit="no_model", samples=2000, degenerate=2000), "all"))
# (with real counts among the -1s a model always exists: status 0, and the degenerate samples must not stop the scan)
CASES.append(_coinciding("half_sources_coincide", T(status=0, degenerate=lambda d: d >= 20, samples=lambda s: s >= 100,
                                                    instalments=lambda i: i >= 1), "half"))


def _all_inliers():
    name = "all_inliers"
    rng = _rng(name)
    src = rng.integers(0, 1500, (500, 2)).astype(np.float64)
    dst = np.stack([-src[:, 1], src[:, 0]], 1) + SHIFT           # a quarter turn: exact on the pixel lattice
    return Case(name, *embed(rng, src, dst, 500, np.arange(500)), T(samples=1, winner=0, winner_count=500, status=0),
                exact=np.array([[0.0, -1.0, 17.0], [1.0, 0.0, -9.0]]))


CASES.append(_all_inliers())
for _s in (1, 12345):
    CASES.append(sample_case("seed_%d" % _s, T(status=0, samples=lambda s: s >= 10), 400, 0.3, 1.2, data_seed=5, seed=_s))
CASES.append(sample_case("confidence_0.5", T(status=0, samples=lambda s: 2 <= s < 20), 400, 0.3, 1.2, data_seed=5, confidence=0.5))
CASES.append(sample_case("confidence_0.999999", T(status=0, samples=lambda s: s > 100), 400, 0.3, 1.2, data_seed=5,
                         confidence=0.999999))


def _thr_case(thr):
    """Pairs under one exact model whose residuals are 0, EXACTLY thr^2 (not inliers: the comparison is strict) and the
    largest lattice value below thr^2 (inliers), and outliers.  thr 1, 5, 10: an integer translation, offsets (1, 0) | (3, 4)
    | (6, 8), (10, 0) against (0, 0) | (2, 4) | (7, 7).  thr 0.5: a scaling by 1/2 -- exact for even source coordinates, a
    residual of exactly 1/2 for an odd x; below 1/4 the half-pixel lattice has only 0."""
    name = "thr_%s" % thr
    rng = _rng(name)
    n = 400
    kind = np.arange(n) % 8           # 0-3 exact, 4-5 on the threshold, 6 just inside, 7 outlier
    signs = rng.choice([-1.0, 1.0], (n, 2))
    swap = rng.random(n) < 0.5
    if thr == 0.5:
        src = 2.0 * rng.integers(0, 750, (n, 2))
        src[(kind == 4) | (kind == 5), 0] += 1.0
        dst = np.floor(src / 2.0) + SHIFT
        dst[kind == 5, 0] += 1.0          # residual -1/2 and +1/2
    else:
        on, inside = {1.0: ((1, 0), (0, 0)), 5.0: ((3, 4), (2, 4)), 10.0: ((6, 8), (7, 7))}[thr]
        src = rng.integers(0, 1500, (n, 2)).astype(np.float64)
        off = np.zeros((n, 2))
        off[(kind == 4) | (kind == 5)] = on
        if thr == 10.0:
            off[kind == 5] = (10, 0)
        off[kind == 6] = inside
        off = np.where(swap[:, None], off[:, ::-1], off) * signs
        dst = src + SHIFT + off
    dst[kind == 7] = rng.integers(0, 1500, (int((kind == 7).sum()), 2))
    n_on = int(((kind == 4) | (kind == 5)).sum())
    return Case(name, *embed(rng, src, dst, n, np.arange(n)), T(status=0, boundary=lambda b: b is not None and b >= n_on),
                thr=thr)


CASES += [_thr_case(t) for t in (0.5, 1.0, 5.0, 10.0)]
# (data seeds and sigmas found by search over 0.5 .. 3.0; the predicates prove the round counts)
REFINE = {"0": (0, 0.5), "1": (1, 1.0), "3plus": (2, 1.5), "cap": (10, 2.5)}
for _k, _want in (("0", 0), ("1", 1), ("3plus", lambda r: r is not None and 3 <= r < 10), ("cap", 10)):
    CASES.append(sample_case("refine_rounds_%s" % _k, T(status=0, rounds=_want), 300, 0.6, REFINE[_k][1], data_seed=REFINE[_k][0]))
CASES.append(sample_case("refine_big", T(status=0, n_good=3100, rounds=lambda r: r >= 1), 3100, 0.7, 2.0))

# ---- coordinates ---------------------------------------------------------------------------------------------------------
_neg = lambda m: all(t < 0 for t in m) and any(t != np.floor(t) for t in m)      # noqa: E731
CASES.append(sample_case("negative_coords", T(status=0, means=_neg), 300, 0.6, 1.2, lo=-1500, hi=0))
CASES.append(sample_case("negative_mean_straddling_zero", T(status=0, means=lambda m: _neg(m) and all(t > -100 for t in m),
                                                            pairs=lambda p: all((c > 0).any() and (c < 0).any() for c in p)),
                         300, 0.6, 1.2, lo=-330, hi=270))


def _large(name, n, claim, top=4194304.0):
    """n pairs under an exact quarter turn (exact in float64 at any magnitude) with |coordinate| up to `top` = 2^22, a few
    outliers among them; the largest magnitude is exactly `top` (one source x), which makes n 8 top^2 = n 2^47."""
    rng = _rng(name)
    src = top - 1000.0 * rng.permutation(4 * n)[:2 * n].reshape(n, 2) - rng.integers(1, 500, (n, 2))
    src[0, 0] = top
    dst = np.stack([-src[:, 1], src[:, 0]], 1) + np.array([500.0, -700.0])
    if n >= 8:
        dst[3::8] += rng.integers(50, 90, (len(dst[3::8]), 2))
    assert np.abs(src).max() == top and np.abs(dst).max() < top and np.abs(src).min() > top / 2
    return Case(name, *embed(rng, src, dst, n, np.arange(n), lo=int(top) - 300000, hi=int(top)), claim,
                exact=np.array([[0.0, -1.0, 500.0], [1.0, 0.0, -700.0]]) if claim.want["status"] == 0 else None)


CASES.append(_large("large_ok", 8, T(status=0, n_good=8)))
CASES.append(_large("large_just_allowed_n63", 63, T(status=0, n_good=63)))                     # 63 2^47 < 2^53
CASES.append(_large("large_refused_n64", 64, T(status=3, n_good=64, exit="magnitude")))        # 64 2^47 = 2^53
CASES.append(_large("large_refused_n65", 65, T(status=3, n_good=65, exit="magnitude")))


def _odd_coordinate(name, claim, value, on_good, side):
    rng = _rng(name)
    nq = 300
    good_at = np.arange(0, nq, 2)
    src = rng.integers(0, 1500, (len(good_at), 2)).astype(np.float64)
    idx, dist_sq, qpts, tpts = embed(rng, src, src + SHIFT, nq, good_at)
    for q in (40, 140) if on_good else (41, 141, 299):
        if side == "query":
            qpts[q, 1] = value
        else:
            tpts[idx[q, 0], 0] = value
    return Case(name, idx, dist_sq, qpts, tpts, claim, exact=SHIFT_M if claim.want["status"] == 0 else None)


CASES.append(_odd_coordinate("coord_2p24", T(status=3, exit="not_integer", n_good=150), 16777216.0, True, "query"))
CASES.append(_odd_coordinate("coord_minus_2p24_train", T(status=3, exit="not_integer", n_good=150), -16777216.0, True, "train"))
CASES.append(_odd_coordinate("fraction_on_bad_match", T(status=0, exit="ok", n_good=150), 77.5, False, "query"))
CASES.append(_odd_coordinate("fraction_on_bad_match_train", T(status=0, exit="ok", n_good=150), 77.5, False, "train"))
CASES.append(_odd_coordinate("fraction_on_good_match", T(status=3, exit="not_integer", n_good=150), 77.5, True, "query"))
CASES.append(_odd_coordinate("fraction_on_good_match_train", T(status=3, exit="not_integer", n_good=150), 77.5, True, "train"))

BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


# ---- the checks ------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_complete():
    assert len(CASES) == len(BY_NAME) == N_CASES


@pytest.mark.parametrize("name", NAMES)
def test_each_case_meets_the_boundary_it_claims(name):
    c = BY_NAME[name]
    mat, n_good, status, trace = expected(c)
    assert (n_good, status) == (trace["n_good"], trace["status"]) and (mat is None) == (status != 0)
    assert trace["ratio_path"] == MR.ratio_path(len(c.idx), c.max_iters)
    shown = {k: v for k, v in trace.items() if k not in ("good", "mask", "pairs")}
    assert c.claim(trace), (name, shown)
    if c.exact is not None:
        assert status == 0 and np.array_equal(mat, c.exact), (name, mat)


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_projects_definition(name):
    """match_ref against sparse_cpu.estimate_affine_partial_2d over the good matches (numpy's float32 ratio test, as
    feature_detection.match_features states it), np.array_equal; None in the same cases."""
    c = BY_NAME[name]
    mat, n_good, status, trace = expected(c)
    dist = np.sqrt(c.dist_sq)
    good = np.nonzero((dist[:, 0] < F32(c.ratio) * dist[:, 1]) & (c.idx[:, 0] >= 0) & (c.idx[:, 0] < c.n_train))[0]
    assert n_good == len(good)
    if status in (1, 3):
        assert len(good) < 3 if status == 1 else len(good) >= 3
        return
    exp, mask = SP.estimate_affine_partial_2d(c.qpts[good], c.tpts[c.idx[good, 0]].astype(F32), c.confidence, c.thr, c.max_iters,
                                              c.seed)
    if exp is None:
        assert status == 2 and mat is None
    else:
        assert status == 0 and np.array_equal(mat, exp), (name, mat, exp)
        assert np.array_equal(mask, trace["mask"])


@pytest.mark.parametrize("name", NAMES)
def test_final_fit_is_the_least_squares_solution_of_a_fixed_point(name):
    """The matrix against the uncentred normal equations over the final inliers in rational arithmetic (the tolerance of
    test_feature_reg.py::test_similarity_fit_is_the_least_squares_solution); the final mask is what the matrix selects, unless
    the ten-round cap ended the loop."""
    c = BY_NAME[name]
    mat, _, status, trace = expected(c)
    if status != 0:
        return
    sx, sy, dx, dy = trace["pairs"]
    m = trace["mask"]
    x, y, u, v = ([int(t) for t in col[m]] for col in (sx, sy, dx, dy))
    n = len(x)
    Sx, Sy, Su, Sv = sum(x), sum(y), sum(u), sum(v)
    Sxx = sum(p * p + q * q for p, q in zip(x, y))
    Sxu = sum(p * r + q * t for p, q, r, t in zip(x, y, u, v))
    Sxv = sum(p * t - q * r for p, q, r, t in zip(x, y, u, v))
    D = Fraction(n * Sxx - (Sx * Sx + Sy * Sy))
    a, b = (n * Sxu - (Sx * Su + Sy * Sv)) / D, (n * Sxv - (Sx * Sv - Sy * Su)) / D
    tx, ty = (Su - (a * Sx - b * Sy)) / n, (Sv - (b * Sx + a * Sy)) / n
    exact = np.array([[float(a), float(-b), float(tx)], [float(b), float(a), float(ty)]])
    assert np.allclose(mat, exact, rtol=1e-13, atol=1e-12), (name, np.abs(mat - exact).max())
    if trace["rounds"] < MR.REFINE_CAP:
        assert np.array_equal(SP._similarity_inliers(mat, sx, sy, dx, dy, c.thr * c.thr), m), name
