"""-m gpu: every device call against stale scratch memory.

A call works in memory it does not own for long -- the grow-only workspace of its context, the buffers of the C-side cache,
the small device buffer for taps and scalars, the page-locked buffer for scalar results, and the same set of the companion
context of ma_optflow_register.  The rule is that a call writes every byte before it reads it ("A call
initialises what it reads").  The rest of the suite cannot see a breach: fresh device memory reads as zero, and a call
repeated at one geometry finds the right values of its previous run.

Every case of the registry (tests/_gpu_cases) builds its inputs and its expected result once and then runs its call four
times on the session context: warm (workspace and cache grow to their final size), after Context.debug_fill_idle(0xFF) (NaN as float
and double, -1 / UINT_MAX as integers, 255 as uint8), after debug_fill_idle(0x7F) (3.4e38 as float: finite, so min / max
and comparisons do not drop it as they drop a NaN), and after debug_fill_idle(0x00), the control.  Context.empty is wrapped
so that every array it hands out holds the current poison byte: an output element that a kernel never writes shows.  Each
of the four results must satisfy what the primitive's own GPU test asserts against its statement (the oracle or the
tests/_*_ref.py module, imported from there), and the four must be bit-identical to each other.  Context._run is wrapped
too: the C entries a case declares must be among those it called (tests/test_debug_fill.py checks that the declared entries
and EXEMPT together are every entry of the bindings).

Two further tests run without the hook, in the order production runs: a larger call, then a smaller one on the same
context, the smaller one checked against its statement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.register_assert_rewrite("_gpu_cases")       # the cases' own asserts are quoted by run_case: keep them informative
from _gpu_cases import CASES, POISONS, Env, _O, _RO, assert_same, dev, pair  # noqa: E402
from _gpu_cases.flows import KINDS  # noqa: E402
from _gpu_cases.whole_path import REGISTER  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def env(ctx, tmp_path_factory):
    return Env(ctx, tmp_path_factory)


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
