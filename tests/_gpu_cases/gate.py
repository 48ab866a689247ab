"""Cases of the registry: the gate."""
import numpy as np

from .registry import F32, F64, SHAPE, _O, assert_same, case, dev, labels_u8


@case("nmi_scores, nmi_scores_pair[chunks 0, 10000, 9973]", ("ma_nmi_u8", "ma_nmi_u8_pair"), bits=True)
def _(env):
    O = _O()
    ctx = env.ctx
    a, b0, b1 = (labels_u8(300, 310, s) for s in (1, 2, 3))
    b0[:150] = a[:150]      # a score well away from that of independent labels
    chunks = (0, 10000, 9973)       # 9973 is not a multiple of the kernel's 16-byte loads

    def statement(x, y, chunk):
        fx, fy = x.ravel(), y.ravel()
        if chunk == 0:
            return np.array([O.nmi_u8(x, y)])
        return np.array([O.nmi_u8(fx[i:i + chunk], fy[i:i + chunk]) for i in range(0, fx.size, chunk)])
    exp = {c: (statement(a, b0, c), statement(a, b1, c)) for c in chunks}

    def run():
        da, d0, d1 = dev(ctx, a, b0, b1)
        return {c: (ctx.nmi_scores(da, d0, c), ctx.nmi_scores(da, d1, c)) + ctx.nmi_scores_pair(da, d0, d1, c) for c in chunks}

    def check(got):
        # the tolerance of test_nmi_matches_oracle_and_sklearn (tests/test_gpu_primitives.py): |score - oracle| < 1e-12
        for c in chunks:
            s0, s1, p0, p1 = got[c]
            assert_same((p0, p1), (s0, s1), f"pair against single, chunk {c}")
            for g, e in zip((s0, s1), exp[c]):
                assert g.shape == e.shape
                np.testing.assert_allclose(g, e, rtol=0, atol=1e-12)
    return run, check


@case("nmi_scores[2100 x 2100: the single-band kernel]", "ma_nmi_u8")
def _(env):
    O = _O()
    ctx = env.ctx
    a, b = labels_u8(2100, 2100, 4), labels_u8(2100, 2100, 5)
    b[:, :1000] = a[:, :1000]
    exp = O.nmi_u8(a, b)

    def check(got):
        assert got.shape == (1,) and abs(got[0] - exp) < 1e-12      # test_nmi_matches_oracle_and_sklearn's tolerance
    return (lambda: ctx.nmi_scores(*dev(ctx, a, b), 0)), check


def _cells_of(h, w, cell):
    ch, cw = cell
    return [[(slice(i, min(i + ch, h)), slice(j, min(j + cw, w))) for j in range(0, w, cw)] for i in range(0, h, ch)]


@case("qc_nmi_grid[one image, two images]", "ma_qc_nmi_grid")
def _(env):
    O = _O()
    ctx = env.ctx
    h, w = SHAPE
    cell = (32, 100)
    ref, b1 = labels_u8(h, w, 11), labels_u8(h, w, 12)
    b0 = np.clip(ref.astype(np.int32) + np.random.default_rng(13).integers(-60, 60, (h, w)), 0, 255).astype(np.uint8)
    sl = _cells_of(h, w, cell)
    nmi = [np.array([[O.nmi_u8(np.ascontiguousarray(ref[s]), np.ascontiguousarray(b[s])) for s in row] for row in sl])
           for b in (b0, b1)]
    ncc = [np.array([[np.corrcoef(ref[s].ravel().astype(F64), b[s].ravel().astype(F64))[0, 1] for s in row] for row in sl])
           for b in (b0, b1)]

    def run():
        d = dev(ctx, ref, b0, b1)
        return ctx.qc_nmi_grid(d[0], d[1], None, *cell), ctx.qc_nmi_grid(*d, *cell)

    def check(got):
        one, two = got
        assert one[1] is None and one[3] is None
        assert_same((one[0], one[2]), (two[0], two[2]), "b1 NULL against b1 given")
        # |score - sklearn| <= 1e-12 (test_nmi_constant_cells_and_sklearn) and |r - corrcoef| <= 1e-12 (test_ncc_matches_corrcoef),
        # tests/test_registration_qc.py
        for g, e in zip((two[0], two[1]), nmi):
            assert g.shape == e.shape and np.abs(g - e).max() <= 1e-12
        for g, e in zip((two[2], two[3]), ncc):
            assert g.shape == e.shape and np.abs(g - e).max() <= 1e-12
    return run, check


@case("qc_flow_grid", "ma_qc_flow_grid")
def _(env):
    from test_gpu_flow_smooth import make_flow, odd_values
    from test_registration_qc import np_flow_stats
    ctx = env.ctx
    f, rng = make_flow(*SHAPE)
    f = odd_values(f, rng)
    cell = (32, 100)
    exp = np_flow_stats(f, cell)

    def check(got):
        # assert_flow_stats of tests/test_registration_qc.py: everything equal, flow_mean at rtol = 1e-12
        jmin, folded, invalid, mean, mx = got
        assert np.array_equal(jmin, exp["jac_min"]) and np.array_equal(folded, exp["folded"])
        assert np.array_equal(invalid, exp["invalid"])
        assert np.array_equal(mx.astype(F32), exp["flow_max"], equal_nan=True)
        fin = np.isfinite(exp["flow_mean"])
        assert np.array_equal(fin, np.isfinite(mean))
        np.testing.assert_allclose(mean[fin], exp["flow_mean"][fin], rtol=1e-12, atol=0)
    return (lambda: ctx.qc_flow_grid(dev(ctx, f), *cell)), check


@case("residual_shift_grid", "ma_residual_shift_grid")
def _(env):
    from _residual_shift_ref import residual_shift_ref
    from test_gpu_residual_shift import KEYS, noisy_roll
    ctx = env.ctx
    h, w = SHAPE
    rng = np.random.default_rng(25)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b0, b1 = noisy_roll(rng, a, 1, -3), rng.integers(0, 256, (h, w), dtype=np.uint8)
    cell, R = (40, 150), 4
    exp = tuple({k: e[k] for k in KEYS} for e in (residual_shift_ref(a, b0, cell, R), residual_shift_ref(a, b1, cell, R)))

    def run():
        d = dev(ctx, a, b0, b1)
        two = ctx.residual_shift_grid(*d, *cell, R, table=True)
        one = ctx.residual_shift_grid(d[0], d[2], None, *cell, R, table=True)
        assert one[1] is None
        return two, one[0]
    return run, (exp, exp[1])


@case("translation_moments, translation_search", ("ma_translation_moments", "ma_translation_search"))
def _(env):
    import _translation_ref as T
    ctx = env.ctx
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, SHAPE, dtype=np.uint8)
    b = np.roll(a, (2, -5), axis=(0, 1))
    b[::3] = rng.integers(0, 256, b[::3].shape, dtype=np.uint8)
    window = (-310, 310, -9, 9)         # shifts without an overlap on both sides of x
    res, table = T.search(a, b, window, 2)
    exp = (T.moments(a, b, window), dict(res, table=table))

    def run():
        d = dev(ctx, a, b)
        return ctx.translation_moments(*d, window), ctx.translation_search(*d, window, exclude=2, table=True)
    return run, exp
