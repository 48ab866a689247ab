"""The feature stage at chunk, capacity, window and tiny-image edges: case builders, expected values and the checks that
both are right (CPU only).  tests/test_gpu_feature_edges.py runs the cases on the device and imports everything from here.

Every expectation is one of
  * oracle/feature_oracle.py (fast_detect, daisy_describe -- pinned by the scikit-image fixtures),
  * the host-cut windows of tile_registration.split_image_into_tiles,
  * numpy's stable argsort(-score)[:limit] over the oracle's score map (or over the ANALYTIC map of a dot tile, which a
    test below pins to the oracle),
and every comparison is np.array_equal.

The numbers of csrc/daisy.hip the case lists are built around are restated here as plain numbers (a kernel that changes one
of them has to revisit the lists): the selection works on chunks of 4096 scores, 16 consecutive scores per collecting thread,
passes of 256 chunks in kp_cut_kernel, at most 8192 keys per tile, 16 sorting waves that own 64-aligned stretches of the key
list; the smoothing works on blocks of 64 columns and 4 waves x 16 (or 32) outputs, on content rectangles dilated by the
halo 1, 1 + r0, 1 + r0 + r1 that the input of each of the three smoothings has accumulated.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import feature_oracle as FO
from microaligner_amd.feature_reg import feature_detection as FD
from microaligner_amd.feature_reg import tile_registration as TR
from microaligner_amd.feature_reg.sparse_cpu import Daisy

KC_E, KC_CH, KC_PASS, KS_CAP, KS_WAVES = 16, 4096, 256, 8192, 16       # selection (see the module docstring)
ST_B, SM_NY, SM_SW = 64, 16, 4                                            # smoothing: columns, outputs per thread and step, waves
OV = FD.TILE_OVERLAP


# ---- 0. controlled score maps ------------------------------------------------------------------------------------------
def make_dot_tile(Pi, margin, positions, values, threshold=1):
    """A tile of single bright pixels on a zero background and its non-maximum-suppressed FAST map in closed form: a pixel
    of value v alone on zeros scores v - 1 (all 16 ring pixels are darker by v; the score is the largest threshold that
    keeps the corner), nothing else scores (a zero pixel sees at most one bright ring pixel, not nine).  positions: (n, 2)
    interior (x, y), at least 3 px inside the interior and 4 px apart (Chebyshev); values: 2 .. 255."""
    pos = np.asarray(positions, np.int64).reshape(-1, 2)
    val = np.asarray(values, np.int64).reshape(-1)
    assert len(pos) == len(val)
    P = Pi + 2 * margin
    tile, amap = np.zeros((P, P), np.uint8), np.zeros((Pi, Pi), np.int32)
    if len(pos):
        assert pos.min() >= 3 and pos.max() < Pi - 3 and val.min() >= 2 and val.max() <= 255
        idx = np.sort(pos[:, 1] * Pi + pos[:, 0])
        assert (np.diff(idx) > 0).all()
        # 4 px apart: every dot's 7 x 7 neighbourhood holds no other dot
        dots = np.zeros((Pi, Pi), np.int32)
        dots[pos[:, 1], pos[:, 0]] = 1
        near = sum(dots[pos[:, 1] + dy, pos[:, 0] + dx] for dy in range(-3, 4) for dx in range(-3, 4))
        assert near.max() == 1
        tile[pos[:, 1] + margin, pos[:, 0] + margin] = val
        amap[pos[:, 1], pos[:, 0]] = np.where(val > threshold, val - 1, 0)
    return tile, amap


def grid_positions(Pi, pitch, rows=None):
    """(x, y) of the pitch grid that starts 3 px inside the interior, row-major."""
    c = np.arange(3, Pi - 3, pitch)
    ys, xs = np.meshgrid(c if rows is None else np.asarray(rows), c, indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], 1)


def expected_selection(amap, limit):
    """feature_detection.py:105-106 on a score map: corners in the detector's row-major order, stably sorted by descending
    response, cut to the limit -> (n, 3) int32 rows of x, y, score."""
    ys, xs = np.nonzero(amap)
    sc = amap[ys, xs]
    order = np.argsort(-sc, kind="stable")[:limit]
    return np.stack([xs[order], ys[order], sc[order]], 1).astype(np.int32)


def cut_of(amap, limit):
    """(s*, need_eq, corners at s*, corners): the cut-off score, how many corners of exactly that score the selection takes."""
    sc = amap[amap > 0]
    if len(sc) <= limit:
        return 0, 0, 0, len(sc)
    sstar = int(np.sort(sc)[::-1][limit])          # the strongest corner that does not fit
    gt = int((sc > sstar).sum())
    return sstar, limit - gt, int((sc == sstar).sum()), len(sc)


def selection_mismatch(count, kp, expected, n_corners, limit):
    """None when (count, kp[:count]) is the expected selection, else what is wrong.  count / kp: one tile of
    Context.fast_keypoints."""
    if int(count) != min(n_corners, limit):
        return f"count {int(count)} != min({n_corners}, {limit})"
    if len(expected) != int(count):
        return f"expected list has {len(expected)} rows, count is {int(count)}"
    got = np.asarray(kp)[:int(count)]
    if not np.array_equal(got, expected):
        bad = np.nonzero((got != expected).any(1))[0]
        return f"{len(bad)} rows differ, first at {bad[0]}: got {got[bad[0]]}, expected {expected[bad[0]]}"
    return None


class SelCase:
    """One tile of a selection test."""

    def __init__(self, name, Pi, positions, values, limit, threshold=1, margin=3):
        self.name, self.Pi, self.limit, self.threshold, self.margin = name, Pi, int(limit), threshold, margin
        self.tile, self.amap = make_dot_tile(Pi, margin, positions, values, threshold)
        self.n = int((self.amap > 0).sum())
        self.sstar, self.need_eq, self.n_eq, _ = cut_of(self.amap, self.limit)
        self.expected = expected_selection(self.amap, self.limit)

    def last_tie(self):
        """Row-major index of the last corner of score s* the selection takes, and of the first one it leaves."""
        flat = self.amap.ravel()
        ties = np.nonzero(flat == self.sstar)[0]
        return (int(ties[self.need_eq - 1]) if self.need_eq else None), int(ties[self.need_eq])

    def __repr__(self):
        return self.name


def _mixed(n, seed):
    return np.random.default_rng(seed).integers(2, 256, n)


def _spread(Pi, pitch, n, seed):
    """n positions of the pitch grid, spread over the whole interior (row-major order)."""
    g = grid_positions(Pi, pitch)
    keep = np.sort(np.random.default_rng(seed).choice(len(g), n, replace=False))
    return g[keep]


PI_COUNT = 371                 # pitch 4: 92 x 92 = 8464 grid points >= 8193
COUNT_NS = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193)


@functools.lru_cache(maxsize=None)
def count_case(n):
    return SelCase(f"count{n}", PI_COUNT, _spread(PI_COUNT, 4, n, 100 + n), _mixed(n, 200 + n), KS_CAP)


N_LIMIT = 501


@functools.lru_cache(maxsize=None)
def limit_case(limit):
    return SelCase(f"limit{limit}", 203, _spread(203, 4, N_LIMIT, 7), _mixed(N_LIMIT, 8), limit)


def _two_levels(n_hi, n_lo, v_hi, v_lo, seed):
    pos = _spread(203, 4, n_hi + n_lo, seed)
    val = np.full(n_hi + n_lo, v_lo)
    val[np.random.default_rng(seed + 1).choice(n_hi + n_lo, n_hi, replace=False)] = v_hi
    return pos, val


@functools.lru_cache(maxsize=None)
def tie_case(name):
    if name == "all_equal":
        return SelCase(name, 203, _spread(203, 4, 500, 11), np.full(500, 100), 300)
    if name in ("need_eq_0", "need_eq_1", "need_eq_all_but_one"):
        pos, val = _two_levels(200, 300, 200, 50, 12)
        return SelCase(name, 203, pos, val, {"need_eq_0": 200, "need_eq_1": 201, "need_eq_all_but_one": 499}[name])
    if name in ("cut_at_score_1", "cut_at_score_254", "scores_1_and_254_inside"):
        pos, val = _two_levels(100, 400, 255, 2, 13)
        if name == "scores_1_and_254_inside":
            val = val.copy()
            val[::3] = _mixed(len(val[::3]), 14)
            return SelCase(name, 203, pos, val, 450)
        return SelCase(name, 203, pos, val, 250 if name == "cut_at_score_1" else 50)
    if name == "threshold_100":
        return SelCase(name, 203, _spread(203, 4, 500, 15), _mixed(500, 16), 150, threshold=100)
    raise KeyError(name)


TIE_CASES = ("all_equal", "need_eq_0", "need_eq_1", "need_eq_all_but_one", "cut_at_score_1", "cut_at_score_254",
             "scores_1_and_254_inside", "threshold_100")

PI_EDGE = 403                  # 403^2 = 162409 = 39 * 4096 + 2665 = 16 * 10150 + 9: a partial last chunk that reaches dot rows


def _edge_population():
    """Equal dots at pitch 4 on every second grid row plus the last row a dot may sit on (which lies in the final, partial
    chunk); every seventh dot is stronger, so that the chunk bases carry a share above the cut as well."""
    rows = list(range(3, PI_EDGE - 3, 8))
    if PI_EDGE - 4 - rows[-1] >= 4:
        rows.append(PI_EDGE - 4)
    pos = grid_positions(PI_EDGE, 4, rows)
    val = np.full(len(pos), 90)
    val[::7] = 180
    return pos, val


def _straddling_limit(boundary, after):
    """The limit at which the last tie taken is the last one before (after=False) or the first one behind (after=True) a
    multiple of `boundary` in row-major index that two consecutive ties straddle, about two thirds into the tile."""
    pos, val = _edge_population()
    idx = pos[:, 1] * PI_EDGE + pos[:, 0]
    ties = np.sort(idx[val == 90])
    k = np.nonzero(ties[1:] // boundary - ties[:-1] // boundary == 1)[0]
    gap = ties[k + 1] - ties[k]
    k = k[gap == gap.min()]                        # neighbours in a row where there are any
    k = int(k[2 * len(k) // 3])
    n_hi = int((val == 180).sum())
    return n_hi + k + 1 + (1 if after else 0), int(ties[k]), int(ties[k + 1])


@functools.lru_cache(maxsize=None)
def edge_case(name):
    pos, val = _edge_population()
    if name == "final_chunk":
        limit = len(pos) - 3
    else:
        kind, side = name.rsplit("_", 1)
        limit = _straddling_limit({"thread": KC_E, "chunk": KC_CH}[kind], side == "after")[0]
    return SelCase(name, PI_EDGE, pos, val, limit)


EDGE_CASES = ("thread_before", "thread_after", "chunk_before", "chunk_after", "final_chunk")

PI_BIG = 1040                  # 1040^2 / 4096 = 264.06: 265 chunks, a second pass of kp_cut_kernel


@functools.lru_cache(maxsize=None)
def big_case(name):
    pos = grid_positions(PI_BIG, 16)
    if name == "all_equal":
        return SelCase("big_" + name, PI_BIG, pos, np.full(len(pos), 77), len(pos) - 40)
    val = np.full(len(pos), 50)
    val[::3] = 200
    return SelCase("big_" + name, PI_BIG, pos, val, len(pos) - 40)


BIG_CASES = ("all_equal", "two_levels")


@functools.lru_cache(maxsize=None)
def multi_tiles():
    """An all-zero tile, a constant one, two corners, a full grid of ties, 8193 mixed corners: (tiles, maps)."""
    P = PI_COUNT + 6
    full = grid_positions(PI_COUNT, 4)
    dots = [make_dot_tile(PI_COUNT, 3, count_case(2).expected[:, :2], count_case(2).expected[:, 2] + 1),
            make_dot_tile(PI_COUNT, 3, full, np.full(len(full), 33)),
            (count_case(8193).tile, count_case(8193).amap)]
    tiles = [np.zeros((P, P), np.uint8), np.full((P, P), 7, np.uint8)] + [d[0] for d in dots]
    maps = [np.zeros((PI_COUNT, PI_COUNT), np.int32)] * 2 + [d[1] for d in dots]
    return tiles, maps


NMS_CASES = [(Pi, m) for Pi in (255, 256, 257, 1, 6, 7) for m in (0, 3)]


def noise_image(shape, seed, sigma=1.2):
    """Smoothed noise scaled to 0 .. 255: corners everywhere, thin strips included."""
    from scipy.ndimage import gaussian_filter
    img = gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma)
    span = img.max() - img.min()
    return np.round((img - img.min()) / (span if span > 0 else 1.0) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def nms_case(Pi, margin):
    """(tile, expected map): smoothed noise; the 7 px interior carries a bright pixel at its only scorable position."""
    tile = noise_image((Pi + 2 * margin, Pi + 2 * margin), 1000 + Pi + margin)
    if Pi == 7:
        tile = (tile // 2).astype(np.uint8)
        tile[margin + 3, margin + 3] = 250
    return tile, FO.fast_detect(tile, margin, 1) if margin else FO.fast_nms(FO.fast_score(tile, 1))


# ---- 2. windows and descriptors ----------------------------------------------------------------------------------------
TILE = 100                     # windows of 202
RADII = tuple(len(h) - 1 for h in FD._daisy_tables(Daisy(radius=21, q_radius=3, q_theta=8, q_hist=8))[0])
HALOS = (1, 1 + RADII[0], 1 + RADII[0] + RADII[1])       # what the input of each smoothing has accumulated


def _spans():
    """Content extents at which the dilated input (span + 2 h) of a smoothing is 63, 64 or 65 columns wide."""
    out = []
    for h in HALOS:
        out += [s for s in (ST_B - 1 - 2 * h, ST_B - 2 * h, ST_B + 1 - 2 * h) if 1 <= s < TILE]
    return out


SPANS = _spans()
SINGLE_SHAPES = ([(SPANS[(i + 4) % len(SPANS)], w) for i, w in enumerate(SPANS)] + [(1, 1), (1, 99), (99, 1), (7, 7)])   # (H, W)
REMAINDER_SHAPES = [(151, 201), (250, 152), (251, 299), (201, 151), (152, 250), (299, 200), (200, 101)]
REMAINDERS = (1, 50, 51, 52, 99, 100)
DENSE_SHAPE = (351, 352)       # 4 x 4 windows, ragged remainders


def strip_image(shape, seed):
    """Smoothed noise plus bright pixels 3 .. 6 px inside the image border (where the image is large enough to hold them)."""
    H, W = shape
    img = (noise_image(shape, seed).astype(np.int32) * 200 // 255).astype(np.uint8)
    for k, d in enumerate((3, 4, 5, 6)):
        for y, x in ((d, 3 + 8 * k), (3 + 8 * k, d), (H - 1 - d, W - 4 - 8 * k), (H - 4 - 8 * k, W - 1 - d)):
            if 0 <= y < H and 0 <= x < W:
                img[y, x] = 255
    return img


def smoothing_waves(span_h, span_w, n_windows, radius, halo, nit, P=TILE + 2 * OV):
    """smooth_pair's wave count: what decides between 16 and 32 outputs per thread."""
    in_h, in_w = min(P, span_h + 2 * halo), min(P, span_w + 2 * halo)
    out_h = min(P, in_h + 2 * radius)
    return -(-in_w // ST_B) * -(-out_h // (SM_NY * nit)) * n_windows * 8


def window_contents(shape, tile=TILE):
    """(y0, y1, x0, x1) of the image inside every window, in window coordinates."""
    H, W = shape
    P = tile + 2 * OV
    out = []
    for ty in range(-(-H // tile)):
        for tx in range(-(-W // tile)):
            wy, wx = ty * tile - OV, tx * tile - OV
            out.append((max(0, -wy), min(P, H - wy), max(0, -wx), min(P, W - wx)))
    return out


class Extracted:
    """Combined features of an image as tile_registration.find_features lays them out."""

    def __init__(self, pts, resp, desc, counts, windows):
        self.pts, self.resp, self.desc, self.counts, self.windows = pts, resp, desc, counts, windows


def expected_features(img, limit, tile=TILE, describe=True):
    """The statement of ma_feature_extract from the oracle: host-cut windows; per window fast_detect and the stable selection;
    windows with fewer than three keypoints dropped; points = window origin + interior coordinate; descriptors =
    daisy_describe(window, interior coordinates)."""
    windows, info = TR.split_image_into_tiles(img, tile)
    ntx = info["ntiles"]["x"]

    def one(t):
        sel = expected_selection(FO.fast_detect(windows[t], OV, 1), limit)
        if len(sel) < 3:
            return len(sel), None
        p = sel[:, :2].astype(np.float64)
        des = FO.daisy_describe(windows[t], p) if describe else np.zeros((len(p), 200), np.float32)
        return len(sel), (p + np.array([t % ntx * tile, t // ntx * tile], np.float64), sel[:, 2].astype(np.int32), des)

    with ThreadPoolExecutor(max_workers=8) as ex:
        per = list(ex.map(one, range(len(windows))))
    kept = [r for _, r in per if r is not None]
    counts = [c for c, _ in per]
    if not kept:
        return Extracted(np.zeros((0, 2)), np.zeros(0, np.int32), np.zeros((0, 200), np.float32), counts, windows)
    return Extracted(np.concatenate([k[0] for k in kept]), np.concatenate([k[1] for k in kept]),
                     np.concatenate([k[2] for k in kept]), counts, windows)


def features_mismatch(got, exp):
    """None when the (pts, resp, desc) triple `got` equals the expectation bit for bit, else what differs."""
    pts, resp, desc = got
    if len(pts) != len(exp.pts):
        return f"{len(pts)} keypoints, expected {len(exp.pts)}"
    if not np.array_equal(pts, exp.pts):
        return "points differ"
    if not np.array_equal(resp, exp.resp):
        return "responses differ"
    if desc.shape != exp.desc.shape or not np.array_equal(desc, exp.desc):
        bad = np.nonzero((np.asarray(desc) != exp.desc).any(1))[0]
        return f"descriptors of {len(bad)} keypoints differ, first {bad[0]} at {exp.pts[bad[0]]}"
    return None


LIMIT = 24


@functools.lru_cache(maxsize=None)
def single_case(shape):
    img = strip_image(shape, 31 * shape[0] + shape[1])
    return img, expected_features(img, LIMIT)


@functools.lru_cache(maxsize=None)
def capacity_case():
    """One window whose few hundred corners all fit the largest limit there is (KS_CAP)."""
    img = strip_image((99, 99), 3)
    return img, expected_features(img, KS_CAP)


@functools.lru_cache(maxsize=None)
def remainder_case(shape):
    img = strip_image(shape, 17 * shape[0] + shape[1])
    return img, expected_features(img, 12)


@functools.lru_cache(maxsize=None)
def dense_case():
    img = strip_image(DENSE_SHAPE, 5)
    return img, expected_features(img, 12)


DROP_COUNTS = (0, 5, 4, 1, 2, 3, 6, 2)      # corners per window of a 1 x 8 image: dropped ones first and last of a pair, and of all


@functools.lru_cache(maxsize=None)
def drop_image():
    img = np.zeros((TILE, TILE * len(DROP_COUNTS)), np.uint8)
    rng = np.random.default_rng(9)
    for t, n in enumerate(DROP_COUNTS):
        for k in range(n):       # weak corners: the oracle's brute-force score walks every threshold up to the strongest
            y, x = 3 + 13 * k + int(rng.integers(0, 4)), 3 + 15 * k + int(rng.integers(0, 5))
            img[y, t * TILE + x] = int(rng.integers(8, 40))
    return img


@functools.lru_cache(maxsize=None)
def drop_case(limit):
    return expected_features(drop_image(), limit)


DROP_LIMITS = (40, 6, 5, 2)


# ---- 3. FeatureRegistrator on tiny images --------------------------------------------------------------------------------
TINY_SHAPES = [(1, 1), (1, 300), (300, 1), (7, 150), (150, 7), (60, 60), (99, 99), (151, 201)]


def tiny_pair(shape, dtype):
    """A textured image and the same content moved by (+3, -2) px, cut from one larger field."""
    H, W = shape
    field = noise_image((H + 8, W + 8), 7 * H + W, sigma=1.5).astype(np.float64)
    field = field * (257.0 if np.dtype(dtype) == np.uint16 else 1.0)
    return field[4:4 + H, 4:4 + W].astype(dtype), field[6:6 + H, 1:1 + W].astype(dtype)


# ---- the checks of this file ---------------------------------------------------------------------------------------------
def test_the_analytic_map_of_a_dot_tile_is_the_oracles():
    """One pixel of value v alone on zeros scores v - 1 and nothing else scores: values 2 and 255, dots exactly 3 px from the
    interior's border, pitches 4 to 8, thresholds 1 and 100, margins 0 and 3 -- against feature_oracle.fast_detect."""
    rng = np.random.default_rng(0)
    for pitch, Pi in ((4, 59), (5, 64), (6, 101), (7, 200), (8, 77)):
        pos = grid_positions(Pi, pitch)
        assert pos.min() == 3 and (pos.max() == Pi - 4 or pitch > 4)
        val = rng.integers(2, 256, len(pos))
        val[:2], val[-2:] = (2, 255), (255, 2)
        for margin, thr in ((3, 1), (0, 1), (3, 100))[:1 if Pi == 200 else 3]:     # (the brute-force score is slow at 200 px)
            tile, amap = make_dot_tile(Pi, margin, pos, val, thr)
            assert np.array_equal(FO.fast_detect(tile, margin, thr) if margin else FO.fast_nms(FO.fast_score(tile, thr)), amap)
            assert (amap > 0).sum() == (val > thr).sum() and amap.max() == 254 and (thr > 1 or amap[amap > 0].min() == 1)
    corner = np.array([[3, 3], [55, 3], [3, 55], [55, 55]])          # Pi = 59: 3 px from every border
    tile, amap = make_dot_tile(59, 3, corner, [2, 255, 9, 100])
    assert np.array_equal(FO.fast_detect(tile, 3, 1), amap) and (amap > 0).sum() == 4
    with pytest.raises(AssertionError):
        make_dot_tile(59, 3, [[3, 3], [6, 5]], [9, 9])                # closer than 4 px
    with pytest.raises(AssertionError):
        make_dot_tile(59, 3, [[2, 3]], [9])                           # on the 3 px border


def test_the_selection_cases_meet_the_boundaries_they_claim():
    for n in COUNT_NS:
        c = count_case(n)
        assert c.n == n and c.limit == KS_CAP and len(c.expected) == min(n, KS_CAP)
        assert n < 64 or len(np.unique(c.amap[c.amap > 0])) > 30        # mixed values: ties and distinct scores
    assert count_case(8193).need_eq >= 1 and count_case(8192).sstar == 0 == count_case(8192).need_eq
    # chunks of every count case: the dots are spread over all of them
    big = count_case(8193)
    assert len(np.unique(np.nonzero(big.amap.ravel())[0] // KC_CH)) == -(-PI_COUNT * PI_COUNT // KC_CH)
    for limit in (1, N_LIMIT - 1, N_LIMIT, N_LIMIT + 1):
        c = limit_case(limit)
        assert c.n == N_LIMIT and len(c.expected) == min(limit, N_LIMIT)
    got = {k: (tie_case(k).sstar, tie_case(k).need_eq, tie_case(k).n_eq, tie_case(k).n) for k in TIE_CASES}
    assert got["all_equal"] == (99, 300, 500, 500)
    assert got["need_eq_0"] == (49, 0, 300, 500) and got["need_eq_1"] == (49, 1, 300, 500)
    assert got["need_eq_all_but_one"] == (49, 299, 300, 500)
    assert got["cut_at_score_1"] == (1, 150, 400, 500) and got["cut_at_score_254"] == (254, 50, 100, 500)
    c = tie_case("scores_1_and_254_inside")
    assert {1, 254} <= set(c.expected[:, 2].tolist()) and c.n > c.limit and c.sstar == 1
    c = tie_case("threshold_100")
    assert c.n < 500 * 0.7 and c.amap[c.amap > 0].min() == 100 and c.n > c.limit and c.need_eq >= 1
    # thread, chunk and sorting-wave boundaries
    npx = PI_EDGE * PI_EDGE
    assert npx % KC_E and npx % KC_CH and (PI_COUNT * PI_COUNT) % KC_E and 401 * 401 % KC_E == 1
    for kind, B in (("thread", KC_E), ("chunk", KC_CH)):
        _, a, b = _straddling_limit(B, False)
        assert a // B + 1 == b // B
        before, after = edge_case(kind + "_before"), edge_case(kind + "_after")
        assert before.last_tie() == (a, b) and after.last_tie()[0] == b and after.limit == before.limit + 1
        assert before.sstar == after.sstar == 89 and 0 < before.need_eq < before.n_eq - 1
    c = edge_case("final_chunk")
    last, nxt = c.last_tie()
    nch = -(-npx // KC_CH)
    assert last // KC_CH == nxt // KC_CH == nch - 1 and npx - (nch - 1) * KC_CH < KC_CH and c.n == c.limit + 3
    for name in EDGE_CASES:                  # ties at the cut in more than one sorting wave's stretch of the key list
        c = edge_case(name)
        sel = c.expected[np.argsort(c.expected[:, 1] * c.Pi + c.expected[:, 0])]      # the key list: row-major
        per = (-(-len(sel) // KS_WAVES) + 63) // 64 * 64
        assert len(np.unique(np.nonzero(sel[:, 2] == c.sstar)[0] // per)) >= 8
    # more than 256 chunks
    nch = -(-PI_BIG * PI_BIG // KC_CH)
    assert nch == 265 > KC_PASS
    for name in BIG_CASES:
        c = big_case(name)
        last, nxt = c.last_tie()
        ties = np.nonzero(c.amap.ravel() == c.sstar)[0]
        assert last // KC_CH >= KC_PASS and nxt // KC_CH >= KC_PASS and 4000 < c.n == c.limit + 40 <= KS_CAP
        assert (ties // KC_CH < KC_PASS).sum() > 1000 and (ties // KC_CH >= KC_PASS).sum() > 40
        if name == "two_levels":
            hi = np.nonzero(c.amap.ravel() > c.sstar)[0]
            assert (hi // KC_CH < KC_PASS).sum() > 1000 and (hi // KC_CH >= KC_PASS).sum() > 10
    tiles, maps = multi_tiles()
    assert [int((m > 0).sum()) for m in maps] == [0, 0, 2, 8464, 8193] and len({t.shape for t in tiles}) == 1
    assert np.array_equal(FO.fast_detect(tiles[1][:80, :80], 3, 1), np.zeros((74, 74), np.int32))


def test_the_small_score_maps_have_what_they_claim():
    tile, exp = nms_case(7, 3)
    assert exp.shape == (7, 7) and (exp > 0).sum() == 1 and exp[3, 3] > 0
    for Pi in (1, 6):
        assert not nms_case(Pi, 0)[1].any() and nms_case(Pi, 3)[1].shape == (Pi, Pi)
    assert (nms_case(257, 0)[1][:, 253:] > 0).any() and (nms_case(255, 3)[1] > 0).sum() > 500


def test_the_window_shapes_meet_the_block_edges_they_claim():
    assert RADII == (11, 18, 23) and HALOS == (1, 12, 30)
    assert SPANS == [61, 62, 63, 39, 40, 41, 3, 4, 5]
    widths, heights = {s[1] for s in SINGLE_SHAPES}, {s[0] for s in SINGLE_SHAPES}
    for h, r in zip(HALOS, RADII):
        for axis in (widths, heights):
            assert {ST_B - 1, ST_B, ST_B + 1} <= {s + 2 * h for s in axis}                     # the dilated input
            if h + r < ST_B // 2:
                assert {ST_B - 1, ST_B, ST_B + 1} <= {s + 2 * h + 2 * r for s in axis}         # the outputs of the pass
    assert all(h != w for h, w in SINGLE_SHAPES[:len(SPANS)]) and {(1, 1), (1, 99), (99, 1), (7, 7)} <= set(SINGLE_SHAPES)
    # content narrower than a halo; the dilated rectangle clipped by the window on the left / top only
    assert min(SPANS) < HALOS[1] and OV < HALOS[2] + RADII[2] and OV + max(SPANS) + HALOS[2] + RADII[2] < TILE + 2 * OV
    # remainders of the last column and row
    rows = {H - (-(-H // TILE) - 1) * TILE for H, _ in REMAINDER_SHAPES}
    cols = {W - (-(-W // TILE) - 1) * TILE for _, W in REMAINDER_SHAPES}
    assert rows == set(REMAINDERS) == cols
    for shape in REMAINDER_SHAPES:
        assert 4 <= len(window_contents(shape)) <= 9
    # below 51 the second-to-last window's content stops short of its end, at 51 it fills it exactly
    P = TILE + 2 * OV
    assert window_contents((100, 150))[0][3] == P - 1 and window_contents((100, 151))[0][3] == P == window_contents((100, 152))[0][3]
    # both smoothing schedules: one batch of 16 windows takes 32 outputs per thread, batches of one or two take 16
    cont = window_contents(DENSE_SHAPE)
    span_h, span_w = max(c[1] - c[0] for c in cont), max(c[3] - c[2] for c in cont)
    assert len(cont) == 16 and len({(c[1] - c[0], c[3] - c[2]) for c in cont}) >= 9            # ragged rectangles
    for h, r in zip(HALOS, RADII):
        assert smoothing_waves(span_h, span_w, 16, r, h, 2) >= 3 * 1024 > smoothing_waves(span_h, span_w, 2, r, h, 2)
        assert smoothing_waves(span_h, span_w, 13, r, h, 2) < 3 * 1024


def test_the_feature_cases_have_keypoints_where_they_should():
    for shape in SINGLE_SHAPES:
        img = strip_image(shape, 31 * shape[0] + shape[1])
        n = expected_features(img, LIMIT, describe=False).counts[0]
        # nothing scores within 3 px of the window's interior; a 7 x 7 image keeps two corners: a dropped window
        assert n == 0 if min(shape) < 4 else n == 2 if shape == (7, 7) else n >= 10, (shape, n)
    assert sum(1 for s in SINGLE_SHAPES if min(s) >= 4 and max(s) >= 39) == 7
    exp = expected_features(drop_image(), 40, describe=False)
    assert tuple(exp.counts) == DROP_COUNTS and len(exp.pts) == sum(c for c in DROP_COUNTS if c >= 3)
    assert max(DROP_COUNTS) in DROP_LIMITS and max(DROP_COUNTS) - 1 in DROP_LIMITS
    assert len(expected_features(drop_image(), 2, describe=False).pts) == 0                     # every window dropped
    n = expected_features(strip_image((99, 99), 3), KS_CAP, describe=False).counts[0]
    assert 256 < n < KS_CAP                                    # more than one block of the compaction, fewer than the limit
    exp = expected_features(strip_image((151, 201), 17 * 151 + 201), 12, describe=False)
    assert exp.counts == [12, 12, 0, 12, 12, 0]          # nothing scores in a last column of one pixel


def test_the_tiny_pairs_are_a_shift():
    for shape in TINY_SHAPES:
        for dt in (np.uint8, np.uint16):
            ref, mov = tiny_pair(shape, dt)
            assert ref.shape == mov.shape == shape and ref.dtype == dt
            if shape[0] > 2 and shape[1] > 3:
                assert np.array_equal(ref[2:, :-3], mov[:-2, 3:]) and ref.max() > 0


# ---- 4. teeth --------------------------------------------------------------------------------------------------------------
def test_the_selection_comparison_catches_rank_errors():
    """The comparison the device tests use reports a selection whose ties are swapped, whose last tie is the next one in
    row-major order, or that misses one chunk's share -- and passes the right one."""
    c = edge_case("chunk_before")
    good = c.expected
    kp = np.zeros((c.limit + 5, 3), np.int32)
    kp[:c.limit] = good
    assert selection_mismatch(c.limit, kp, good, c.n, c.limit) is None
    ties = np.nonzero(good[:, 2] == c.sstar)[0]
    swapped = good.copy()
    swapped[[ties[3], ties[4]]] = swapped[[ties[4], ties[3]]]
    assert "rows differ" in selection_mismatch(c.limit, kp, swapped, c.n, c.limit)
    _, nxt = c.last_tie()
    moved = good.copy()
    moved[-1] = (nxt % c.Pi, nxt // c.Pi, c.sstar)
    assert good[-1, 2] == c.sstar and "rows differ" in selection_mismatch(c.limit, kp, moved, c.n, c.limit)
    chunk = (good[:, 1] * c.Pi + good[:, 0]) // KC_CH
    short = good[chunk != 5]
    assert 0 < len(short) < len(good) and selection_mismatch(c.limit, kp, short, c.n, c.limit) is not None
    assert selection_mismatch(c.limit - 1, kp, good, c.n, c.limit) is not None


def test_the_descriptor_comparison_catches_a_shifted_window():
    """Descriptors computed from a window whose content sits one column off are reported."""
    img, exp = single_case((40, 61))
    got = (exp.pts.copy(), exp.resp.copy(), exp.desc.copy())
    assert len(exp.pts) >= 3 and features_mismatch(got, exp) is None
    shifted = np.roll(exp.windows[0], 1, axis=1)
    bad = FO.daisy_describe(shifted, exp.pts)
    assert "descriptors" in features_mismatch((exp.pts, exp.resp, bad), exp)
    assert "points" in features_mismatch((exp.pts + [1.0, 0.0], exp.resp, exp.desc), exp)
    assert features_mismatch((exp.pts[:-1], exp.resp[:-1], exp.desc[:-1]), exp) is not None
