"""-m gpu: every device call against stale scratch memory.

A call works in memory it does not own for long -- the grow-only workspace of its context, the buffers of the C-side cache,
the small device buffer for taps and scalars, the page-locked buffer for scalar results, and the same set of the companion
context of ma_optflow_register.  The rule is that a call writes every byte before it reads it ("A call
initialises what it reads").  The rest of the suite cannot see a breach: fresh device memory reads as zero, and a call
repeated at one geometry finds the right values of its previous run.

Every case of the registry below builds its inputs and its expected result once and then runs its call four times on the
session context: warm (workspace and cache grow to their final size), after Context.debug_fill_idle(0xFF) (NaN as float
and double, -1 / UINT_MAX as integers, 255 as uint8), after debug_fill_idle(0x7F) (3.4e38 as float: finite, so min / max
and comparisons do not drop it as they drop a NaN), and after debug_fill_idle(0x00), the control.  Context.empty is wrapped
so that every array it hands out holds the current poison byte: an output element that a kernel never writes shows.  Each
of the four results must satisfy what the primitive's own GPU test asserts against its statement (the oracle or the
tests/_*_ref.py module, imported from there), and the four must be bit-identical to each other.  Context._run is wrapped
too: the C entries a case declares must be among those it called (tests/test_debug_fill.py checks that the declared entries
and EXEMPT together are every entry of the bindings).

Two further tests run without the hook, in the order production runs: a larger call, then a smaller one on the same
context, the smaller one checked against its statement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
POISONS = (0xFF, 0x7F, 0x00)

# C entries that launch no kernel over scratch memory: the cap on what the registry may leave out
EXEMPT = {
    "ma_version": "a string",
    "ma_last_error": "a string",
    "ma_device_count": "device query",
    "ma_device_info": "device query",
    "ma_ctx_create": "context call",
    "ma_ctx_destroy": "context call",
    "ma_ctx_stream": "context call",
    "ma_ctx_trim": "context call: frees the caches",
    "ma_ctx_transfer_stats": "context call: reads two host counters",
    "ma_ctx_set_workspace_limit": "option call",
    "ma_ctx_set_option": "option call",
    "ma_ctx_get_option": "option call",
    "ma_sync": "context call: waits for the stream",
    "ma_malloc": "allocation",
    "ma_free": "allocation",
    "ma_memset": "fills caller memory",
    "ma_memcpy_h2d": "copy between caller buffers",
    "ma_memcpy_d2h": "copy between caller buffers",
    "ma_memcpy_d2d": "copy between caller buffers",
    "ma_memcpy_d2h_async": "copy between caller buffers",
    "ma_host_alloc": "host memory",
    "ma_host_free": "host memory",
    "ma_host_register": "host memory",
    "ma_host_unregister": "host memory",
    "ma_host_transfer_is_direct": "host memory query",
    "ma_host_parallel_copy": "host copy",
    "ma_host_stream_copy": "host copy",
    "ma_host_pcg64_choice2": "host arithmetic, no ctx",
    "ma_host_ransac_iterations": "host arithmetic, no ctx",
    "ma_host_np_mean": "host arithmetic, no ctx",
    "ma_transient_pin_stats": "host counters of the page-locking of caller memory, no ctx",
    "ma_translation_scores": "host arithmetic on a table of moments, no ctx (include/microaligner_translation.h)",
    "ma_event_create": "event call",
    "ma_event_destroy": "event call",
    "ma_event_record": "event call",
    "ma_event_elapsed_ms": "event call",
    "ma_event_sync": "event call",
    "ma_engine_memcpy_h2d": "engine call: copy between caller buffers through the staging rings",
    "ma_engine_memcpy_d2h": "engine call: copy between caller buffers through the staging rings",
    "ma_engine_record": "engine call",
    "ma_engine_wait": "engine call",
    "ma_engine_sync": "engine call",
    "ma_profile_enable": "profile call",
    "ma_profile_reset": "profile call",
    "ma_profile_get": "profile call",
    "ma_clock_probe": "a spin kernel that touches no memory",
    "ma_params_default": "fills a host struct",
    "ma_warp_pages_plan": "host arithmetic, no ctx",
    "ma_debug_fill_idle": "the hook itself",
}


# ---- the registry ----------------------------------------------------------------------------------------------------------
class Case:
    """name; the C entries the case exercises; make(env) -> (run, expected): run() makes the call(s) and returns the
    results as numpy arrays / scalars in tuples, lists or dicts; expected is the same structure (compared bit for bit, NaN
    standing for NaN) or a function check(result) where the primitive's own test uses a tolerance.  bits: whether the four
    results must be bit-identical to each other."""

    def __init__(self, name, entries, make, bits=True):
        self.name, self.entries, self.make, self.bits = name, tuple(entries), make, bits


CASES = []


def case(name, entries, bits=True):
    if isinstance(entries, str):
        entries = (entries,)

    def deco(make):
        assert name not in [c.name for c in CASES], name
        CASES.append(Case(name, entries, make, bits))
        return make
    return deco


def declared_entries():
    return {e for c in CASES for e in c.entries}


class Env:
    """what make() gets: the context, and the restatements that are compiled once per module"""

    def __init__(self, ctx, tmp_path_factory):
        self.ctx, self._tmp, self._made = ctx, tmp_path_factory, {}
        self.poison = POISONS[0]         # the byte Context.empty and the cases' host outputs are filled with

    def _once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    @property
    def interp(self):
        from _remap_interp_ref import InterpRef
        return self._once("interp", lambda: InterpRef(self._tmp.mktemp("stale_interp_ref")))

    @property
    def levels(self):
        from _fb_levels_ref import LevelsRef
        return self._once("levels", lambda: LevelsRef(self._tmp.mktemp("stale_levels_ref")))


@pytest.fixture(scope="module")
def env(ctx, tmp_path_factory):
    return Env(ctx, tmp_path_factory)


def assert_same(got, exp, where=""):
    """the same structure and the same bits, any NaN payload standing for NaN"""
    if isinstance(exp, dict):
        assert isinstance(got, dict) and set(got) == set(exp), where
        for k in exp:
            assert_same(got[k], exp[k], f"{where}[{k!r}]")
    elif isinstance(exp, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(exp), where
        for k, (g, e) in enumerate(zip(got, exp)):
            assert_same(g, e, f"{where}[{k}]")
    elif exp is None:
        assert got is None, where
    elif isinstance(exp, np.ndarray):
        # float arrays by their bits, hence of one dtype; integer and bool arrays by their values (flags come back as bool)
        assert isinstance(got, np.ndarray) and got.shape == exp.shape and \
            (got.dtype == exp.dtype or "f" not in (got.dtype.kind, exp.dtype.kind)), \
            f"{where}: {getattr(got, 'dtype', type(got))} {getattr(got, 'shape', None)} against {exp.dtype} {exp.shape}"
        if exp.dtype.kind == "f":
            gn, en = np.isnan(got), np.isnan(exp)
            assert np.array_equal(gn, en), f"{where}: NaN masks differ at {np.argwhere(gn != en)[:5].tolist()}"
            u = {4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
            bad = np.ascontiguousarray(got).view(u) != np.ascontiguousarray(exp).view(u)
            bad &= ~en
        else:
            bad = got != exp
        assert not bad.any(), f"{where}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[:5].tolist()}"
    elif isinstance(exp, (float, np.floating)):
        assert (got == exp) or (got != got and exp != exp), f"{where}: {got!r} against {exp!r}"
    else:
        assert got == exp, f"{where}: {got!r} against {exp!r}"


def run_case(ctx, monkeypatch, env, c):
    from microaligner_amd import _lib as L
    from microaligner_amd.device import Context
    called, poison = set(), [POISONS[0]]
    env.poison = POISONS[0]
    plain_run, plain_empty = Context._run, Context.empty

    def recording_run(self, fn, *args):
        called.add(fn.__name__)
        return plain_run(self, fn, *args)

    def poisoned_empty(self, shape, dtype):
        a = plain_empty(self, shape, dtype)
        L.check(self.lib.ma_memset(self.handle, a.ptr, poison[0], a._nbytes_alloc))
        return a

    monkeypatch.setattr(Context, "_run", recording_run)
    monkeypatch.setattr(Context, "empty", poisoned_empty)
    run, expected = c.make(env)
    results = []
    for k, byte in enumerate((None,) + POISONS):
        if byte is not None:
            filled = ctx.debug_fill_idle(byte)
            assert len(filled) == 4
            poison[0] = env.poison = byte
        results.append(run())
        ctx.sync()
    passes = ("warm", "after 0xFF", "after 0x7F", "after 0x00")
    failed = []                 # every pass is judged, so that a failure says which passes it is a failure of
    for k, res in enumerate(results):
        try:
            if callable(expected):
                expected(res)
            else:
                assert_same(res, expected, passes[k])
        except AssertionError as e:
            failed.append(f"{passes[k]}: against the statement: {str(e).splitlines()[0] if str(e) else repr(e)}")
        if c.bits and k:
            try:
                assert_same(res, results[0], passes[k])
            except AssertionError as e:
                failed.append(f"{passes[k]}: against the warm pass: {str(e).splitlines()[0] if str(e) else repr(e)}")
    assert not failed, f"{len(failed)} checks failed:\n" + "\n".join(failed)
    missing = set(c.entries) - called
    assert not missing, f"declared but never called: {sorted(missing)} (called: {sorted(called)})"


# ---- inputs ----------------------------------------------------------------------------------------------------------------
SHAPE = (67, 301)       # ragged against every tile of the library, more than one block along x


def pair(h, w, seed, dtype=np.float32, **kw):
    from microaligner_amd import synthetic
    return synthetic.make_pair(h, w, seed, dtype, **kw)


def labels_u8(h, w, seed):
    """random labels over all 256 values"""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def dev(ctx, *arrays):
    out = tuple(None if a is None else ctx.asdevice(a) for a in arrays)
    return out[0] if len(out) == 1 else out


# ---- Farneback -----------------------------------------------------------------------------------------------------------
def _farneback(name, shape, win, iters, seed, oracle, **kw):
    @case(name, "ma_farneback_tiled")
    def make(env):
        ctx = env.ctx
        ref, mov = pair(*shape, seed=seed)
        exp = oracle(ref, mov)
        return (lambda: ctx.farneback(*dev(ctx, mov, ref), win, iters, **kw).numpy()), exp


def _O():
    from oracle import oracle as O
    return O


def _RO():
    from oracle import register_oracle as RO
    return RO


_farneback("farneback[untiled]", (131, 157), 19, 3, 150, lambda ref, mov: _O().calc_optical_flow_farneback(mov, ref, 19, 3))
_farneback("farneback[fused]", (140, 150), 31, 3, 8,
           lambda ref, mov: _O().calc_optical_flow_farneback(mov, ref, 31, 3, fused=True), fused=True)
# ragged right and bottom windows that are mostly padding: what the active-extent and needed-rectangle arguments are about
_farneback("farneback[tiled]", (250, 310), 19, 3, 100, lambda ref, mov: _RO().tile_flow(ref, mov, 100, 20, 19, 3),
           tile=100, overlap=20)
_farneback("farneback[tiled,fused]", (250, 310), 19, 3, 100,
           lambda ref, mov: _RO().tile_flow(ref, mov, 100, 20, 19, 3, fused=True), tile=100, overlap=20, fused=True)
_farneback("farneback[fallback kernels]", (40, 700), 601, 2, 5,
           lambda ref, mov: _O().calc_optical_flow_farneback(mov, ref, 601, 2))


@case("farneback[tiled,batches under an 8 MiB workspace]", "ma_farneback_tiled")
def _(env):
    from microaligner_amd import _lib as L
    ctx = env.ctx
    ref, mov = pair(250, 310, seed=100)
    exp = _RO().tile_flow(ref, mov, 100, 20, 19, 3)

    def run():
        # one 140 x 140 window takes 140 * 192 * 4 * 20 B = 2.05 MiB of planes: 8 MiB forces batches of 3 windows
        L.check(ctx.lib.ma_ctx_set_workspace_limit(ctx.handle, 8 << 20))
        try:
            return ctx.farneback(*dev(ctx, mov, ref), 19, 3, tile=100, overlap=20).numpy()
        finally:
            L.check(ctx.lib.ma_ctx_set_workspace_limit(ctx.handle, 48 << 30))
    return run, exp


@case("farneback[levels=2]", "ma_farneback_levels")
def _(env):
    from test_gpu_farneback_levels import _pair
    ctx = env.ctx
    mov, ref = _pair(131, 157, np.float32)
    exp = env.levels.farneback(mov, ref, 2, 15, 3, fused=False)
    return (lambda: ctx.farneback(*dev(ctx, mov, ref), 15, 3, levels=2).numpy()), exp


@case("farneback_debug", "ma_farneback_debug")
def _(env):
    ctx = env.ctx
    ref, mov = pair(150, 170, 3)
    flow, r0, r1, m0 = _O().calc_optical_flow_farneback(mov, ref, 21, 1, dump=True)
    exp = (flow,) + tuple(np.ascontiguousarray(np.moveaxis(a, 2, 0)) for a in (r0, r1, m0))
    return (lambda: tuple(a.numpy() for a in ctx.farneback_debug(*dev(ctx, mov, ref), 21, 1))), exp


# ---- pyramid, min / max, conversions ---------------------------------------------------------------------------------------
def _image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) * (65535 if dtype == np.uint16 else 255)).astype(dtype)


for _dtype in (np.uint8, np.uint16, np.float32):
    def _pyr(dtype=_dtype):
        tag = np.dtype(dtype).name

        @case(f"pyr_down[{tag}]", "ma_pyr_down")
        def _(env):
            ctx = env.ctx
            img = _image(SHAPE, dtype, 67)
            return (lambda: ctx.pyr_down(dev(ctx, img)).numpy()), _O().pyr_down(img)

        @case(f"pyr_down[{tag},minmax]", "ma_pyr_down_minmax")
        def _(env):
            ctx = env.ctx
            img = _image(SHAPE, dtype, 68)
            exp = _O().pyr_down(img)

            def run():
                p = ctx.pyr_down(dev(ctx, img), minmax=True)
                return p.numpy(), p.minmax.numpy()
            return run, (exp, np.array([exp.min(), exp.max()], F32))

        @case(f"minmax, normalize_minmax_u8, to_f32[{tag}]",
              ("ma_minmax", "ma_normalize_minmax_u8") + (("ma_convert_f32",) if dtype != np.float32 else ()))
        def _(env):
            ctx = env.ctx
            img = _image(SHAPE, dtype, 69)
            exp = ((float(img.min()), float(img.max())), _O().normalize_minmax_u8(img.astype(F32)), img.astype(F32))

            def run():
                d = dev(ctx, img)
                return ctx.minmax(d), ctx.normalize_minmax_u8(d).numpy(), ctx.to_f32(d).numpy()
            return run, exp

        @case(f"image_quantiles, normalize_range_u8[{tag}]", ("ma_image_quantiles", "ma_normalize_range_u8"))
        def _(env):
            import _quantile_ref as Q
            from test_gpu_quantiles import QSETS, image
            ctx = env.ctx
            img = image((301, 517), dtype)          # of test_gpu_quantiles.SHAPES
            img.ravel()[::97] = 0
            sets = [(q, False) for q in QSETS] + [(QSETS[-1], True)]
            lo, hi = (float(v) for v in Q.image_quantiles(img, [0.01, 0.99])[0])
            exp = [Q.image_quantiles(img, q, z) for q, z in sets] + [Q.normalize_range_u8(img, lo, hi)]

            def run():
                d = dev(ctx, img)
                got = []
                for q, z in sets:
                    vals, counts = ctx.image_quantiles(d, q, ignore_zeros=z)
                    got.append((vals, tuple(counts)))
                return got + [ctx.normalize_range_u8(d, lo, hi).numpy()]
            return run, exp
    _pyr()


@case("pyr_up_flow", "ma_pyr_up_flow")
def _(env):
    from test_gpu_primitives import rand_flow
    ctx = env.ctx
    f = rand_flow(40, 50, 11, 5.0)
    exp = [_O().pyr_up(f * F32(s), dstsize=(99, 79)) for s in (1.0, 2.0, 4.0)]
    return (lambda: [ctx.pyr_up_flow(dev(ctx, f), (79, 99), s).numpy() for s in (1.0, 2.0, 4.0)]), exp


@case("max_project", "ma_max_project")
def _(env):
    ctx = env.ctx
    rng = np.random.default_rng(0)
    stack = rng.integers(0, 60000, (5,) + SHAPE).astype(np.uint16)
    fs = (stack / F32(7)).astype(F32)
    fs[1, 0, 0] = np.nan
    fs[2, 30:40, 10:90] = np.nan
    return (lambda: [ctx.max_project(dev(ctx, s)).numpy() for s in (stack, fs)]), [stack.max(0), np.maximum.reduce(fs)]


# ---- DOG --------------------------------------------------------------------------------------------------------------------
_DT = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}


@case("dog_u8[every entry, every flag, every sigma pair of the suite]", ("ma_dog_u8", "ma_dog_u8_minmax", "ma_dog_u8_ex"))
def _(env):
    O = _O()
    ctx = env.ctx
    h, w = SHAPE
    imgs = [pair(h, w, seed=301, dtype=dt)[0] for dt in (np.uint8, np.uint16, np.float32)]
    sigmas = [(5, 9), (1, 2), (3, 5), (6, 9)]
    flags = [0, O.DOG_FUSED_BLUR, O.DOG_FUSED_SCALE, O.DOG_FUSED]
    exp = {}
    for k, img in enumerate(imgs):
        for s in sigmas:
            for fl in flags:
                exp[k, s, fl] = O.dog(img, True, *s, flags=fl)
        exp[k, "plain"] = (exp[k, (5, 9), 0], 0)
        exp[k, "minmax"] = (exp[k, (5, 9), 0], 0)
    exp["zero"] = (np.zeros((h, w), np.uint8), True)

    def run():
        got = {}
        for k, img in enumerate(imgs):
            d = dev(ctx, img)
            for s in sigmas:
                for fl in flags:
                    got[k, s, fl] = ctx.dog_u8(d, *s, flags=fl).numpy()
            flag = C.c_int(-1)
            out = ctx.empty((h, w), np.uint8)
            ctx._run(ctx.lib.ma_dog_u8, d.ptr, _DT[d.dtype], h, w, 5, 9, out.ptr, C.byref(flag))
            got[k, "plain"] = (out.numpy(), flag.value)
            mm = dev(ctx, np.array([img.min(), img.max()], F32))
            flag = C.c_int(-1)
            out = ctx.empty((h, w), np.uint8)
            ctx._run(ctx.lib.ma_dog_u8_minmax, d.ptr, _DT[d.dtype], h, w, 5, 9, mm.ptr, out.ptr, C.byref(flag))
            got[k, "minmax"] = (out.numpy(), flag.value)
        out, zero = ctx.dog_u8(dev(ctx, np.zeros((h, w), F32)), report_zero=True)
        got["zero"] = (out.numpy(), zero)
        return got
    return run, exp


# ---- the gate ---------------------------------------------------------------------------------------------------------------
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


# ---- warps ------------------------------------------------------------------------------------------------------------------
TILE, OV = 50, 12           # tile > 2 overlap > 0: the tiling has cells; (67, 301) is ragged against it both ways
MODES = ("nearest", "linear", "cubic", "lanczos4")


def _img(shape, dtype, seed):
    from tests.test_gpu_warp_interp import image
    return image(shape[0], shape[1], dtype, seed)


def _flow(shape, seed, amp=6.0):
    from tests.test_gpu_warp_interp import flow_for
    return flow_for(shape[0], shape[1], seed, amp)


@case("remap[every interpolation]", ("ma_remap_bilinear", "ma_remap_interp"))
def _(env):
    from tests.test_gpu_warp_interp import maps
    ctx = env.ctx
    srcs = [_img(SHAPE, dt, 3) for dt in (np.uint8, np.uint16, np.float32)]
    m = maps(70, 90, *SHAPE, 4)["bad"]
    exp = [[_O().remap(s, m) if mode == "linear" else env.interp.remap(s, m, mode) for mode in MODES] for s in srcs]
    return (lambda: [[ctx.remap(*dev(ctx, s, m), interpolation=mode).numpy() for mode in MODES] for s in srcs]), exp


@case("warp[every interpolation, minmax, flow_cells]",
      ("ma_warp_tiled", "ma_warp_tiled_interp", "ma_warp_tiled_minmax", "ma_warp_tiled_flowcells"))
def _(env):
    ctx = env.ctx
    flow = _flow(SHAPE, 5)
    imgs = [_img(SHAPE, dt, 6) for dt in (np.uint8, np.uint16, np.float32)]
    lin = [_RO().warp(i, flow, TILE, OV) for i in imgs]
    exp = [dict({m: env.interp.warp(i, flow, TILE, OV, m) for m in MODES if m != "linear"}, linear=e,
                minmax=(e, np.array([e.min(), e.max()], F32)), cells=(e, np.array([e.min(), e.max()], F32)))
           for i, e in zip(imgs, lin)]

    def run():
        got = []
        for i in imgs:
            d, f = dev(ctx, i, flow)
            r = {m: ctx.warp(d, f, TILE, OV, interpolation=m).numpy() for m in MODES}
            w = ctx.warp(d, f, TILE, OV, minmax=True)
            r["minmax"] = (w.numpy(), w.minmax.numpy())
            w = ctx.warp(d, f, TILE, OV, minmax=True, flow_cells=True)
            assert f.cellkeys is not None
            r["cells"] = (w.numpy(), w.minmax.numpy())
            got.append(r)
        return got
    return run, exp


@case("warp_pages[every interpolation]", ("ma_warp_pages_host", "ma_warp_pages_host_interp"))
def _(env):
    ctx = env.ctx
    flow = _flow(SHAPE, 7)
    pages = [_img(SHAPE, np.uint16, 40 + k) for k in range(3)]
    exp = {m: [_RO().warp(p, flow, TILE, OV) if m == "linear" else env.interp.warp(p, flow, TILE, OV, m) for p in pages]
           for m in MODES}

    def run():
        f = dev(ctx, flow)
        got = {}
        for m in MODES:
            own = ctx.warp_pages(pages, f, TILE, OV, interpolation=m)
            out = [np.full(SHAPE, env.poison * 257, np.uint16) for _ in pages]
            ctx.warp_pages(pages, f, TILE, OV, out=out, interpolation=m)
            assert_same(out, own, f"caller's pages, {m}")
            got[m] = own
        return got
    return run, exp


def _tmat(H, W):
    from tests.test_warp_compose_ref import rotation
    return rotation(7, (W - 1) / 2, (H - 1) / 2, 0.98, 1.5, -2.0)


@case("warp_affine_flow, warp_affine_flow_pages[every interpolation]", ("ma_warp_affine_flow", "ma_warp_affine_flow_pages_host"))
def _(env):
    from tests._warp_compose_ref import warp_affine_flow
    ctx = env.ctx
    H, W = SHAPE
    flow, tmat = _flow(SHAPE, 8, 3.0), _tmat(H, W)
    pages = [_img((H - 5, W - 8), np.uint16, 50 + k) for k in range(2)]
    exp = {m: [warp_affine_flow(env.interp, p, flow, tmat, m) for p in pages] for m in MODES}

    def run():
        f = dev(ctx, flow)
        got = {}
        for m in MODES:
            got[m] = [ctx.warp_affine_flow(dev(ctx, p), f, tmat, interpolation=m).numpy() for p in pages]
            out = [np.full(SHAPE, env.poison * 257, np.uint16) for _ in pages]
            ctx.warp_affine_flow_pages(pages, f, tmat, out=out, interpolation=m)
            assert_same(out, got[m], f"page driver, {m}")
        return got
    return run, exp


@case("warp_affine_grid, warp_affine_grid_pages[every interpolation]", ("ma_warp_affine_grid", "ma_warp_affine_grid_pages_host"))
def _(env):
    import _flow_grid_ref as G
    from microaligner_amd import FlowGrid
    from tests._warp_compose_ref import warp_affine_flow
    ctx = env.ctx
    H, W, s = 65, 130, 7            # of test_gpu_flow_grid.SHAPES: one row and two columns past the 64 x 32 tile
    nodes = G.sample_ref(G.smooth_flow((H, W), 6, amp=4.0), s)
    dense, tmat = G.expand_ref(nodes, (H, W), s), _tmat(H, W)
    pages = [_img((H - 5, W - 8), np.uint16, 60 + k) for k in range(2)]
    exp = {m: [warp_affine_flow(env.interp, p, dense, tmat, m) for p in pages] for m in MODES}

    def run():
        grid = FlowGrid(dev(ctx, nodes), s, (H, W))
        got = {}
        for m in MODES:
            got[m] = [ctx.warp_affine_grid(dev(ctx, p), grid, tmat, interpolation=m).numpy() for p in pages]
            out = [np.full((H, W), env.poison * 257, np.uint16) for _ in pages]
            ctx.warp_affine_grid_pages(pages, grid, tmat, out=out, interpolation=m)
            assert_same(out, got[m], f"page driver, {m}")
        return got
    return run, exp


@case("warp_affine, warp_affine_cv", ("ma_warp_affine", "ma_warp_affine_cv"))
def _(env):
    from oracle import affine_oracle as A
    ctx = env.ctx
    H, W = SHAPE
    th = np.deg2rad(7.3)
    M = np.array([[np.cos(th), -np.sin(th), 10.4], [np.sin(th), np.cos(th), -21.7]])
    inv = A.inverse_matrix(np.array([[np.cos(th), -np.sin(th), 12.5], [np.sin(th), np.cos(th), -7.25]]))
    imgs = [_image(SHAPE, dt, 7) for dt in (np.uint8, np.uint16, np.float32)]
    exp = [(A.warp_with_inverse(i, inv).astype(i.dtype), _O().warp_affine(i, M), _O().warp_affine(i, M, dsize=(400, 150)))
           for i in imgs]

    def run():
        got = []
        for i in imgs:
            d = dev(ctx, i)
            got.append((ctx.warp_affine(d, inv).numpy(), ctx.warp_affine_cv(d, M).numpy(),
                        ctx.warp_affine_cv(d, M, dsize=(400, 150)).numpy()))
        return got
    return run, exp


# ---- flows ------------------------------------------------------------------------------------------------------------------
@case("merge_flows[window shortcuts, cell maxima from the warps, banded, untiled]",
      ("ma_merge_flows_tiled", "ma_merge_flows_tiled_cells", "ma_warp_tiled_flowcells"))
def _(env):
    from test_gpu_primitives import rand_flow
    RO = _RO()
    ctx = env.ctx
    h, w = SHAPE
    f1, f2 = rand_flow(h, w, 1, 3.0), rand_flow(h, w, 2, 2.0)
    f1[:25, :100] = 0                                # flow1 all zero in some windows
    f1[30:, :70] = -np.abs(f1[30:, :70])              # max == 0 only through the zero padding
    f2[35:, 150:] = 0
    f2[3, 5, 1] = np.nan                              # a window that takes the general branch whatever else it holds
    img = np.random.default_rng(1).random((h, w)).astype(F32)
    geoms = [(TILE, OV), (40, 25), (0, 0)]            # cells; tile <= 2 overlap: the banded reduction; one window
    exp = [RO.merge_flows(f1, f2, t, o) if t else RO.merge_two_flows(f1, f2) for t, o in geoms]
    exp.append(exp[0])

    def run():
        got = [ctx.merge_flows(*dev(ctx, f1, f2), t, o).numpy() for t, o in geoms]
        d1, d2, dimg = dev(ctx, f1, f2, img)
        for d in (d1, d2):
            ctx.warp(dimg, d, TILE, OV, minmax=True, flow_cells=True)
        got.append(ctx.merge_flows(d1, d2, TILE, OV).numpy())
        return got
    return run, exp


@case("compose_flows", "ma_compose_flows")
def _(env):
    import _flow_compose_ref as R
    from test_gpu_flow_compose import flows
    ctx = env.ctx
    pairs = [flows(*SHAPE, kind, seed=5) for kind in ("few_px", "hundreds_px", "integers")]
    pairs[0][1][5, 6] = (np.nan, 1.0)
    pairs[0][1][66, 300] = (-np.inf, np.nan)
    exp = [R.compose_flows_ref(a, b) for a, b in pairs]
    return (lambda: [ctx.compose_flows(*dev(ctx, a, b)).numpy() for a, b in pairs]), exp


@case("invert_flow", "ma_invert_flow")
def _(env):
    import _flow_invert_ref as R
    from test_gpu_flow_invert import make_flow
    ctx = env.ctx
    fs = [make_flow(*SHAPE, kind) for kind in ("smooth", "folding", "non_finite")]
    exp = []
    for f in fs:
        e, res, missed, _ = R.invert_flow_ref(f, 25, 1e-3)
        exp.append((e, e, res, missed))

    def run():
        got = []
        for f in fs:
            d = dev(ctx, f)
            out, info = ctx.invert_flow(d, 25, 1e-3, return_info=True)
            got.append((ctx.invert_flow(d, 25, 1e-3).numpy(), out.numpy(), info.residual.numpy(), info.not_converged))
        return got
    return run, exp


@case("transform_points", "ma_transform_points")
def _(env):
    import _flow_invert_ref as R
    from microaligner_amd.device import affine_flow_params
    from test_gpu_flow_invert import TMAT, make_flow, points
    ctx = env.ctx
    H, W = SHAPE
    f = make_flow(H, W, "smooth")
    pts = points(1000, H, W, 5)
    shape = (H - 21, W - 10)
    _, m6, left, top = affine_flow_params(shape, F32, f.shape, f.dtype, TMAT)
    exp = [R.to_moving_ref(pts, f, None, (0, 0)), R.to_reference_ref(pts, f, None, (0, 0), 30, 1e-4)[:3],
           R.to_moving_ref(pts, f, m6, (left, top)), R.to_reference_ref(pts, f, TMAT.ravel(), (left, top), 30, 1e-4)[:3]]
    exp = [(e[0], e[1].astype(bool), e[2].astype(bool)) for e in exp]

    def run():
        d = dev(ctx, f)
        got = []
        for kw in (dict(), dict(tmat=TMAT, image_shape=shape)):
            for direction in ("to_moving", "to_reference"):
                p, info = ctx.transform_points(pts, d, direction, max_iter=30, tol=1e-4, return_info=True, **kw)
                got.append((p, info.converged, info.inside))
        return got
    return run, exp


@case("flow_grid_sample, flow_grid_expand, flow_grid_error, transform_points[grid]",
      ("ma_flow_grid_sample", "ma_flow_grid_expand", "ma_flow_grid_error", "ma_transform_points_grid"))
def _(env):
    import _flow_grid_ref as G
    from microaligner_amd import FlowGrid
    from test_gpu_flow_grid import grid_points
    ctx = env.ctx
    shape, s, cell, tol = (65, 130), 7, (16, 16), 1 / 32
    f = G.poison(G.smooth_flow(shape, 11), 12)
    nodes = G.sample_ref(f, s)
    clean = G.sample_ref(G.smooth_flow(shape, 15, amp=3.0), s)
    pts = grid_points(shape, s, 16)
    mv, rf = G.to_moving_grid_ref(pts, clean, shape, s), G.to_reference_grid_ref(pts, clean, shape, s, None, (0, 0), 30, 1e-4)
    exp = (nodes, G.expand_ref(nodes, shape, s), tuple(G.error_maps_ref(f, nodes, s, cell, tol)),
           (mv[0], mv[1].astype(bool), mv[2].astype(bool)), (rf[0], rf[1].astype(bool), rf[2].astype(bool)))

    def run():
        d = dev(ctx, f)
        grid = ctx.flow_grid_sample(d, s)
        given = FlowGrid(nodes, s, shape)
        pg = FlowGrid(dev(ctx, clean), s, shape)
        a, ia = ctx.transform_points(pts, pg, "to_moving", return_info=True)
        b, ib = ctx.transform_points(pts, pg, "to_reference", max_iter=30, tol=1e-4, return_info=True)
        return (grid.nodes.numpy(), ctx.flow_grid_expand(given).numpy(), tuple(ctx.flow_grid_error(d, given, *cell, tol)),
                (a, ia.converged, ia.inside), (b, ib.converged, ib.inside))
    return run, exp


KINDS = ("none", "f32", "u8", "cells")

for _r in (2, 128):
    for _kind in KINDS:
        def _smooth(r=_r, kind=_kind):
            @case(f"smooth_flow[r={r},{kind}]", "ma_smooth_flow")
            def _(env):
                import _flow_smooth_ref as R
                from test_gpu_flow_smooth import make_flow, make_weight, taps_of
                ctx = env.ctx
                shape = (65, 129)            # of test_gpu_flow_smooth.SHAPES: one past the 64 x 128 tile either way
                f, rng = make_flow(*shape)
                weight, cells = make_weight(kind, *shape, rng)
                taps = taps_of(r)
                exp = {mode: R.smooth_flow_ref(f, taps, weight, cells, mode, 1e-3) for mode in ("all", "blend")}

                def run():
                    d, dw = dev(ctx, f, weight)
                    got = {}
                    for mode in ("all", "blend"):
                        out, info = ctx.smooth_flow(d, taps, dw, cells, mode, 1e-3, return_info=True)
                        into = ctx.smooth_flow(d, taps, dw, cells, mode, 1e-3, out=ctx.empty(shape + (2,), F32))
                        assert_same(into.numpy(), out.numpy(), "into a poisoned out")
                        got[mode] = (out.numpy(), info.unsupported)
                    return got
                return run, exp
        _smooth()


@case("fold_mask", "ma_flow_fold_mask")
def _(env):
    import _flow_smooth_ref as R
    from test_gpu_flow_smooth import folding_flow, odd_values
    ctx = env.ctx
    f = odd_values(folding_flow(*SHAPE), None)
    exp = [R.fold_mask_ref(f, margin) for margin in (0, 2, 32)]

    def run():
        got = []
        for margin in (0, 2, 32):
            keep, info = ctx.fold_mask(dev(ctx, f), margin, return_info=True)
            got.append((keep.numpy(), tuple(info)))
        return got
    return run, exp


for _kind in KINDS:
    def _median(kind=_kind):
        @case(f"median_flow[{kind}]", "ma_median_flow")
        def _(env):
            import _flow_median_ref as R
            from test_gpu_flow_median import make_flow, make_weight
            ctx = env.ctx
            shape = (40, 257)                # of test_gpu_flow_median.SHAPES: past the 32 x 64 tile either way
            f, rng = make_flow(*shape)
            weight, cells = make_weight(kind, *shape, rng)
            plan = [(2, "outliers", 0.5, False), (2, "all", np.inf, True), (4, "all", 0.5, False)]   # register, generic, r > 3
            exp = []
            for r, mode, thresh, generic in plan:
                m, part, n = R.window_median(f, r, weight, cells)
                exp.append(tuple(R.finish(f, m, part, n, mode, thresh)))

            def run():
                d, dw = dev(ctx, f, weight)
                got = []
                for r, mode, thresh, generic in plan:
                    out, keep, info = ctx.median_flow(d, r, dw, cells, mode, thresh, return_info=True, keep=True, generic=generic)
                    into = ctx.median_flow(d, r, dw, cells, mode, thresh, out=ctx.empty(shape + (2,), F32), generic=generic)
                    assert_same(into.numpy(), out.numpy(), "into a poisoned out")
                    got.append((out.numpy(), keep.numpy(), tuple(info)))
                return got
            return run, exp

        @case(f"fill_flow[{kind}]", "ma_fill_flow")
        def _(env):
            import _flow_fill_ref as R
            from test_gpu_flow_fill import make_flow, make_weight
            ctx = env.ctx
            shape = (65, 129)                # of test_gpu_flow_fill.SHAPES
            f, rng = make_flow(*shape)
            f[rng.random(shape) < 0.02] = np.nan
            weight, cells = make_weight(kind, *shape, rng)
            e, counts, levels = R.fill_flow_ref(f, weight, cells)
            exp = (e, tuple(counts) + (levels,))

            def run():
                d, dw = dev(ctx, f, weight)
                out, info = ctx.fill_flow(d, dw, cells, return_info=True)
                into = ctx.fill_flow(d, dw, cells, out=ctx.empty(shape + (2,), F32))
                assert_same(into.numpy(), out.numpy(), "into a poisoned out")
                return out.numpy(), tuple(info)
            return run, exp
    _median()


@case("texture_maps", "ma_texture_maps")
def _(env):
    import _texture_ref as T
    from test_gpu_flow_smooth import taps_of
    from test_gpu_texture import CELLS, floor_of, make_image
    ctx = env.ctx
    planes = ("lam_min", "lam_max", "weight")
    cases = []
    for r, dtype in ((7, np.uint16), (128, np.uint8), (2, np.float32)):
        img, taps = make_image(65, 129, dtype), taps_of(r)          # (65, 129): of test_gpu_flow_smooth.SHAPES
        floor = floor_of(T.texture_maps_ref(img, taps))
        cases.append((img, taps, floor))
    exp = []
    for img, taps, floor in cases:
        ref = T.texture_maps_ref(img, taps, floor, CELLS)
        exp.append(dict({n: ref[n] for n in planes}, counts=ref["counts"]))

    def run():
        got = []
        for img, taps, floor in cases:
            g = ctx.texture_maps(dev(ctx, img), taps, floor, CELLS, planes)
            got.append(dict({n: g[n].numpy() for n in planes}, counts=g["counts"]))
        return got
    return run, exp


@case("local_correlation", "ma_local_correlation")
def _(env):
    import _local_correlation_ref as R
    from test_gpu_flow_smooth import taps_of
    from test_gpu_local_correlation import CELLS, PLANES, centres, make_pair, make_weight
    ctx = env.ctx
    shape = (65, 129)
    w, mask = make_weight(*shape)
    cases = []
    for r, dtype, weight, kw in ((7, np.uint16, None, {}), (49, np.uint8, w, dict(min_support=0.3, lo=-0.5, hi=0.9)),
                                 (2, np.float32, mask, dict(min_support=0.05))):
        ref, img, floor = make_pair(*shape, dtype)
        cases.append((ref, img, taps_of(r), floor, centres(ref, img), weight, kw))
    exp = []
    for ref, img, taps, floor, c, weight, kw in cases:
        e = R.local_correlation_ref(ref, img, taps, floor, c, weight, cell_size=CELLS, **kw)
        exp.append(dict({n: e[n] for n in PLANES}, counts=e["counts"]))

    def run():
        got = []
        for ref, img, taps, floor, c, weight, kw in cases:
            g = ctx.local_correlation(*dev(ctx, ref, img), taps, floor, c, dev(ctx, weight), cell_size=CELLS, want=PLANES, **kw)
            got.append(dict({n: g[n].numpy() for n in PLANES}, counts=g["counts"]))
        return got
    return run, exp


@case("flow_refine_step", "ma_flow_refine_step")
def _(env):
    import _flow_refine_ref as R
    from test_gpu_flow_refine import floor_of, make_case, taps_of
    ctx = env.ctx
    shape = (65, 129)                        # of test_gpu_flow_refine.SHAPES
    rng = np.random.default_rng(4)
    wf = rng.uniform(0.1, 2, shape).astype(F32)
    wf[rng.random(shape) < 0.2] = 0
    wu = (rng.random(shape) < 0.6).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    cases = [make_case(*shape, dt) + (taps_of(r), floor_of(dt), wt)
             for r, dt, wt in ((12, np.uint8, None), (1, np.uint16, wf), (128, np.float32, wu))]
    exp = []
    for ref, wp, flow, taps, floor, wt in cases:
        e, s = R.step(ref, wp, flow, taps, floor, wt, 1.0)
        exp.append((e, (float(s.step_max), int(s.clamped), int(s.invalid))))

    def run():
        got = []
        for ref, wp, flow, taps, floor, wt in cases:
            d = dev(ctx, ref, wp, flow)
            out, info = ctx.flow_refine_step(*d, taps, floor, dev(ctx, wt), 1.0, return_info=True)
            into = ctx.flow_refine_step(*d, taps, floor, dev(ctx, wt), 1.0, out=ctx.empty(shape + (2,), F32))
            assert_same(into.numpy(), out.numpy(), "into a poisoned out")
            got.append((out.numpy(), (float(info.step_max), int(info.clamped), int(info.invalid))))
        return got
    return run, exp


U = 2.0 ** -53


@case("flow_affine_moments, flow_affine_apply", ("ma_flow_affine_moments", "ma_flow_affine_apply"))
def _(env):
    import _flow_affine_ref as R
    from test_gpu_flow_affine import make_flow, make_weight
    ctx = env.ctx
    H, W = 65, 511                           # of test_gpu_flow_affine.SHAPES: one row and one column past the 64 x 510 tile
    f, rng = make_flow(H, W, odd=True)
    near = np.array([[1.02, 0.003, -0.4], [-0.002, 0.99, 0.3]])
    plan = [("none", None, None, None), ("f32", (32, 50), None, None), ("u8", None, near, 1.5), ("cells", (32, 50), near, 1.5)]
    plan = [(make_weight(kind, H, W, np.random.default_rng(7), cells), cells, prior, clip) for kind, cells, prior, clip in plan]
    exp = [R.moments_ref(f, weight, cells, prior, clip) for weight, cells, prior, clip in plan]
    A = np.array([[0.99, 0.02, 1.5], [-0.015, 1.01, -2.25]])
    applied = R.apply_ref(f, A)

    def run():
        d = dev(ctx, f)
        got = [ctx.flow_affine_moments(d, dev(ctx, weight), cells, prior, clip) for weight, cells, prior, clip in plan]
        out = ctx.flow_affine_apply(d, A)
        into = ctx.flow_affine_apply(d, A, out=ctx.empty((H, W, 2), F32))
        assert_same(into.numpy(), out.numpy(), "into a poisoned out")
        return got, out.numpy()

    def check(got):
        # check_moments of tests/test_gpu_flow_affine.py: counts equal, every sum within (n + 1) 2^-53 sum |term| of the fsum
        moments, out = got
        for (sums, counts), (e, ecounts, eabs) in zip(moments, exp):
            assert np.array_equal(counts, ecounts)
            assert np.all(np.abs(sums - e) <= (ecounts[..., :1] + 1) * U * eabs)
            assert np.all(sums[ecounts[..., 0] == 0] == 0.0)
        assert_same(out, applied, "flow_affine_apply")
    return run, check


@case("direct_affine_moments, mask_weight", ("ma_direct_affine_moments", "ma_direct_mask_weight"))
def _(env):
    import _direct_affine_ref as R
    from test_gpu_direct_affine import images, make_weight
    ctx = env.ctx
    plan = []
    for shape, rd, md, kind, clip in (((96, 161), np.uint16, np.float32, "f32", None), ((37, 515), np.uint8, np.uint16, "u8", 20.0),
                                      ((96, 161), np.float32, np.uint8, "none", None)):
        ref, mov, M = images(shape, rd, md)
        plan.append((ref, mov, M, 0.9, 2.0, make_weight(kind, shape), clip))
    exp = [R.moments_ref(*p) for p in plan]
    mask = plan[1][5]

    def run():
        got = [ctx.direct_affine_moments(*dev(ctx, ref, mov), M, gain, bias, dev(ctx, weight), clip)
               for ref, mov, M, gain, bias, weight, clip in plan]
        return got, ctx.mask_weight(dev(ctx, mask)).numpy()

    def check(got):
        # check_moments of tests/test_gpu_direct_affine.py
        moments, w = got
        for (sums, counts), (e, ecounts, eabs) in zip(moments, exp):
            assert np.array_equal(counts, ecounts), (counts, ecounts)
            assert np.all(np.abs(sums - e) <= (ecounts[0] + 1) * U * eabs)
        assert_same(w, (mask != 0).astype(F32), "mask_weight")
    return run, check


@case("landmark_flow, landmark_points", ("ma_landmark_flow", "ma_landmark_points"))
def _(env):
    import _landmarks_ref as R
    from test_gpu_landmarks import statement_flow, synthetic
    ctx = env.ctx
    H, W, n = 37, 515, 130                   # of test_gpu_landmarks.SHAPES: three blocks of 256 columns, the last ragged
    cw, a6, c, k, r = synthetic(H, W, n, "integer")
    flows = [statement_flow(H, W, n, "integer", stride) for stride in (1, 8)]
    rng = np.random.default_rng(n + 7)
    p = np.concatenate([r, rng.random((400, 2)) * [W - 1, H - 1], (rng.random((150, 2)) - 0.5) * [8 * W, 8 * H]])
    pexp, mag = R.evaluate(cw, a6, c, k, p)

    def run():
        return [ctx.landmark_flow(cw, a6, c, k, (H, W), stride).numpy() for stride in (1, 8)], ctx.landmark_points(cw, a6, c, k, p)

    def check(got):
        # the derived bounds of tests/test_gpu_landmarks.py: check_flow and the points test
        for g, (e, bound) in zip(got[0], flows):
            assert g.dtype == F32 and g.shape == e.shape and np.all(np.isfinite(g))
            assert np.all(np.abs(g.astype(F64) - e) <= bound + 2.0 ** -23 * np.maximum(1.0, np.abs(e)))
        assert got[1].dtype == F64 and got[1].shape == p.shape and np.all(np.isfinite(got[1]))
        assert np.all(np.abs(got[1] - pexp) <= R.bound(mag, n))
    return run, check


# ---- features -------------------------------------------------------------------------------------------------------------
def _tables():
    from microaligner_amd.feature_reg import feature_detection as FD
    from microaligner_amd.feature_reg.sparse_cpu import Daisy
    return FD._daisy_tables(Daisy(radius=21, q_radius=3, q_theta=8, q_hist=8))


@case("cut_tiles, fast_nms, fast_keypoints", ("ma_cut_tiles_u8", "ma_fast_nms", "ma_fast_keypoints"))
def _(env):
    import test_feature_edges_ref as R
    ctx = env.ctx
    img, feat = R.dense_case()               # 4 x 4 windows with ragged remainders
    tile, nms = R.nms_case(257, 3)           # one past a block of 256 threads
    tiles, maps = R.multi_tiles()            # an all-zero tile, a constant one, two corners, 8464 equal ones, 8193 mixed
    stack = np.ascontiguousarray(np.stack(tiles))
    limit = 100

    def run():
        counts, kp = ctx.fast_keypoints(dev(ctx, stack), 3, limit)
        # rows beyond counts[t] are undefined: what is compared is what selection_mismatch compares
        return (ctx.cut_tiles(dev(ctx, img), R.TILE, R.OV, 0, len(feat.windows)).numpy(),
                ctx.fast_nms(dev(ctx, np.ascontiguousarray(tile[None])), 3), counts,
                [kp[t, :counts[t]].copy() for t in range(len(tiles))])

    def check(got):
        windows, score, counts, kps = got
        assert np.array_equal(windows, np.stack(feat.windows))
        assert score.shape == (1, 257, 257) and np.array_equal(score[0], nms)
        for t in range(len(tiles)):
            bad = R.selection_mismatch(counts[t], kps[t], R.expected_selection(maps[t], limit), int((maps[t] > 0).sum()), limit)
            assert bad is None, (t, bad)
    return run, check


@case("daisy_describe", "ma_daisy_describe")
def _(env):
    import test_feature_edges_ref as R
    ctx = env.ctx
    windows, pts, desc = [], [], []
    for shape in ((40, 61), (63, 4)):
        img, feat = R.single_case(shape)
        windows.append(feat.windows[0])
        pts.append(feat.pts)
        desc.append(feat.desc)
    stack = np.ascontiguousarray(np.stack(windows))
    kp_tile = np.concatenate([np.full(len(p), t, np.int32) for t, p in enumerate(pts)])
    kp_xy = np.concatenate(pts)
    return (lambda: ctx.daisy_describe(dev(ctx, stack), kp_tile, kp_xy, *_tables())), np.concatenate(desc)


@case("feature_extract[waited, enqueued, in batches]", ("ma_feature_extract", "ma_feature_extract_enqueue"))
def _(env):
    import test_feature_edges_ref as R
    from test_gpu_feature_edges import _extract
    ctx = env.ctx
    img, feat = R.dense_case()
    rimg, rfeat = R.remainder_case((251, 299))
    P = R.TILE + 2 * R.OV

    def run():
        d, dr = dev(ctx, img, rimg)
        return ([_extract(ctx, d, 12, workspace_bytes=k * 128 * P * P, wait=wait) for k in (0, 2) for wait in (True, False)],
                _extract(ctx, dr, 12))

    def check(got):
        for g in got[0]:
            bad = R.features_mismatch(g, feat)
            assert bad is None, bad
        bad = R.features_mismatch(got[1], rfeat)
        assert bad is None, bad
    return run, check


def _knn(kind, nq, nt, dim):
    @case(f"knn2[{kind},{nq}x{nt}x{dim}]", ("ma_knn2_l2_ex", "ma_knn2_l2"))
    def _(env):
        from microaligner_amd.feature_reg import sparse_cpu as SP
        from test_feature_reg import _knn_case
        ctx = env.ctx
        q, t = _knn_case(kind, nq, nt, dim, seed=nq + nt)
        exp = SP.knn2_sequential(q, t) if nq * nt <= 3000 * 5000 else None

        def run():
            dq, dt = dev(ctx, q, t)
            got = {}
            for mode in ("exact", "filtered", "filtered_f32", "auto"):
                stats = {}
                got[mode] = ctx.knn2(dq, dt, mode=mode, stats=stats) + (stats["uncertified"],)
            idx, dist = ctx.empty((nq, 2), F32), ctx.empty((nq, 2), F32)
            ctx._run(ctx.lib.ma_knn2_l2, dq.ptr, nq, dt.ptr, nt, dim, idx.ptr, dist.ptr)
            got["ma_knn2_l2"] = (idx.numpy().view(np.int32).astype(np.int64), np.sqrt(dist.numpy()))
            return got

        def check(got):
            # test_filtered_knn2_equals_the_exact_search: every mode gives the exact kernel's bits, and those are the float32
            # definition's where that is quick enough to state
            for mode, g in got.items():
                assert_same(g[:2], got["exact"][:2], mode)
            if exp is not None:
                assert_same(got["exact"][:2], exp, "the float32 definition")
        return run, check


for _args in [("uniform", 1000, 3000, 200), ("uniform", 129, 1000, 200), ("uniform", 1, 2, 200), ("uniform", 300, 5, 8),
              ("uniform", 257, 131, 216), ("uniform", 64, 700, 12), ("histograms", 2500, 4100, 200), ("duplicates", 500, 1500, 200),
              ("near_ties", 200, 900, 200), ("uniform", 6000, 9000, 200), ("wide_range", 700, 2100, 200), ("tiny", 400, 1300, 200),
              ("outlier", 500, 1500, 200), ("clusters", 900, 2600, 200), ("histograms", 333, 1111, 44), ("uniform", 200, 600, 208)]:
    _knn(*_args)


@case("match_similarity", "ma_match_similarity")
def _(env):
    import test_match_ref as R
    from test_gpu_match import _call
    ctx = env.ctx
    names = ("second_instalment", "n_good_1", "large_refused_n64", "max_iters_1", "nq_3100_noisy", "nq_65_noisy")
    exp = [tuple(R.expected(R.BY_NAME[n])[:3]) for n in names]
    return (lambda: [_call(ctx, R.BY_NAME[n]) for n in names]), exp


def _round_images(dtype):
    from microaligner_amd import synthetic
    O = _O()
    H, W = 420, 404
    ref = synthetic.make_cells(H, W, seed=33, dtype=dtype)
    th = np.deg2rad(-0.5)
    mov = O.warp_affine(ref, np.array([[np.cos(th), -np.sin(th), -8.0], [np.sin(th), np.cos(th), 5.0]]))
    return ref, mov


for _use_dog, _dtype in ((True, np.uint16), (False, np.uint8)):
    def _round(use_dog=_use_dog, dtype=_dtype):
        @case(f"feature_round[use_dog={use_dog},{np.dtype(dtype).name}]", "ma_feature_round")
        def _(env):
            from microaligner_amd.feature_reg import feature_detection as FD
            ctx = env.ctx
            tile, chunk = 200, 200 * 200
            ref, mov = _round_images(dtype)
            tables = _tables()

            def step_by_step():
                """the calls ma_feature_round chains, one by one (test_fused_round_equals_the_step_by_step_entry_points)"""
                dref, dmov = dev(ctx, ref, mov)
                ref_gate, gate = ctx.dog_u8(dref), ctx.dog_u8(dmov)
                fr = FD.find_features_of_device_image(ref_gate if use_dog else dref, tile, ctx)
                fm = FD.find_features_of_device_image(gate if use_dog else dmov, tile, ctx)
                idx, dist = ctx.knn2(fm.descriptors_for_search, fr.descriptors_for_search, on_device=True)
                mat, n_good, status = ctx.match_similarity(idx, dist, fm.device_pts(ctx), fr.device_pts(ctx),
                                                           n_train=len(fr.descriptors_for_search))
                assert status == 0 and n_good > 20, (status, n_good)
                cand = ctx.warp_affine_cv(dmov, mat)
                cand_gate = ctx.dog_u8(cand)
                after, before = ctx.nmi_scores_pair(ref_gate, cand_gate, gate, chunk)
                return dict(estimate=mat, n_query=len(fm.descriptors_for_search), n_good=n_good, status=status, after=after,
                            before=before, gate=gate.numpy(), candidate=cand.numpy(), candidate_gate=cand_gate.numpy())
            exp = step_by_step()

            def run():
                dref, dmov = dev(ctx, ref, mov)
                ref_gate = ctx.dog_u8(dref)
                fr = FD.find_features_of_device_image(ref_gate if use_dog else dref, tile, ctx)
                feats = (fr.descriptors_for_search, fr._dev[1], fr._dev[3])
                r = ctx.feature_round(dmov, None, ref_gate, feats, tile, use_dog, chunk, *tables)
                assert not r["zero_max"] and not r["is_identity"]
                return dict(estimate=r["estimate"], n_query=r["n_query"], n_good=r["n_good"], status=r["status"],
                            after=r["scores_after"], before=r["scores_before"], gate=r["current_gate"].numpy(),
                            candidate=r["candidate"].numpy(), candidate_gate=r["candidate_gate"].numpy())
            return run, exp
    _round()


# ---- the whole path -------------------------------------------------------------------------------------------------------------
REGISTER = dict(num_pyr_lvl=2, tile_size=100, overlap=20, use_dog=True)

for _on in (True, False):
    def _register(on=_on):
        @case(f"optflow_register[companion stream {'on' if on else 'off'}]", "ma_optflow_register")
        def _(env):
            ctx = env.ctx
            ref, mov = pair(420, 404, seed=21)
            flow, reports = _RO().register(ref, mov, **REGISTER)
            exp = (flow, [r[3] for r in reports])

            def run():
                ctx.companion_stream = on
                try:
                    f, reps = ctx.optflow_register(*dev(ctx, ref, mov), **REGISTER)
                    return f.numpy(), [r[4] for r in reps], [r[:4] for r in reps]
                finally:
                    ctx.companion_stream = True

            def check(got):
                # test_register_matches_oracle_orchestration: the flow bit for bit, the same levels accepted
                assert_same(got[:2], exp, "register")
            return run, check
    _register()


# ---- the tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_call_on_stale_scratch_memory(ctx, env, monkeypatch, c):
    run_case(ctx, monkeypatch, env, c)


def test_the_hook_fills_what_it_says(ctx):
    """after a call that uses the workspace, the cache, the small device buffer and the page-locked buffer, every kind reports
    bytes; a byte out of range is refused"""
    ref, mov = pair(131, 157, seed=1)
    ctx.optflow_register(*dev(ctx, ref, mov), num_pyr_lvl=1, tile_size=60, overlap=10, use_full_res_img=True)[0].numpy()
    f = dev(ctx, np.zeros((131, 157, 2), F32))
    ctx.merge_flows(f, f, 60, 10).numpy()
    filled = ctx.debug_fill_idle(0)
    assert len(filled) == 4 and all(v > 0 for v in filled), filled
    assert filled[1] % (1 << 16) == 0 and filled[2] % 4096 == 0 and filled[3] % 4096 == 0
    for bad in (-1, 256, 1.0, True):
        with pytest.raises(ValueError):
            ctx.debug_fill_idle(bad)


# ---- production order: a larger call, then a smaller one on the same context ---------------------------------------------
BIG, SMALL = (420, 404), (131, 157)


def test_a_smaller_register_after_a_larger_one(ctx):
    ref, mov = pair(*BIG, seed=21)
    ctx.optflow_register(*dev(ctx, ref, mov), **REGISTER)[0].numpy()
    params = dict(num_pyr_lvl=2, tile_size=60, overlap=10, use_dog=True, use_full_res_img=True)
    ref, mov = pair(*SMALL, seed=22)
    exp, reports = _RO().register(ref, mov, **params)
    flow, reps = ctx.optflow_register(*dev(ctx, ref, mov), **params)
    assert [r[4] for r in reps] == [r[3] for r in reports]
    assert_same(flow.numpy(), exp)


def test_a_smaller_tiled_farneback_after_a_larger_one(ctx):
    ref, mov = pair(*BIG, seed=23)
    ctx.farneback(*dev(ctx, mov, ref), 19, 3, tile=100, overlap=20).numpy()
    ref, mov = pair(*SMALL, seed=24)
    exp = _RO().tile_flow(ref, mov, 60, 10, 9, 3)
    assert_same(ctx.farneback(*dev(ctx, mov, ref), 9, 3, tile=60, overlap=10).numpy(), exp)


def test_a_smaller_dog_after_a_larger_one(ctx):
    for dtype in (np.uint8, np.uint16, np.float32):
        ctx.dog_u8(dev(ctx, pair(*BIG, seed=25, dtype=dtype)[0])).numpy()
        img = pair(*SMALL, seed=26, dtype=dtype)[0]
        assert_same(ctx.dog_u8(dev(ctx, img)).numpy(), _O().dog(img, True))


def test_a_smaller_smooth_flow_after_a_larger_one(ctx):
    import _flow_smooth_ref as R
    from test_gpu_flow_smooth import make_flow, make_weight, taps_of
    for r in (2, 128):
        for kind in KINDS:
            taps = taps_of(r)
            f, rng = make_flow(*BIG)
            weight, cells = make_weight(kind, *BIG, rng)
            ctx.smooth_flow(dev(ctx, f), taps, dev(ctx, weight), cells, "blend", 0.0).numpy()
            f, rng = make_flow(*SMALL)
            weight, cells = make_weight(kind, *SMALL, rng)
            exp, unsupported = R.smooth_flow_ref(f, taps, weight, cells, "blend", 0.0)
            got, info = ctx.smooth_flow(dev(ctx, f), taps, dev(ctx, weight), cells, "blend", 0.0, return_info=True)
            assert_same((got.numpy(), info.unsupported), (exp, unsupported), f"r = {r}, {kind}")


def test_a_smaller_fill_flow_after_a_larger_one(ctx):
    import _flow_fill_ref as R
    from test_gpu_flow_fill import make_flow, make_weight
    for kind in KINDS:
        f, rng = make_flow(*BIG)
        f[rng.random(BIG) < 0.02] = np.nan
        weight, cells = make_weight(kind, *BIG, rng)
        ctx.fill_flow(dev(ctx, f), dev(ctx, weight), cells).numpy()
        f, rng = make_flow(*SMALL)
        f[rng.random(SMALL) < 0.02] = np.nan
        weight, cells = make_weight(kind, *SMALL, rng)
        exp, counts, levels = R.fill_flow_ref(f, weight, cells)
        got, info = ctx.fill_flow(dev(ctx, f), dev(ctx, weight), cells, return_info=True)
        assert_same((got.numpy(), tuple(info)), (exp, tuple(counts) + (levels,)), kind)
