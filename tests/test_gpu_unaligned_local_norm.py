"""-m gpu: ma_normalize_local on stale scratch memory and at unaligned device addresses.

This file adds the cases of the local contrast normalisation to the registry of tests/test_gpu_stale_memory.py at import and
runs exactly those through that file's run_case (warm, then after the idle scratch memory was filled with 0xFF, 0x7F and
0x00: the four results must be the statement's and each other's bits) and through run_shifted of tests/test_gpu_unaligned.py
(the plain allocator, then every array at the edge of what the alignment rule of include/microaligner_hip.h allows).  Below
the rule -- an image, a float32 weight or a float32 output that is not aligned to its element -- the entry returns MA_EINVAL
and names the argument before it launches anything; a uint8 array has no address below the rule.

The file name is load-bearing: it sorts behind test_gpu_stale_memory.py and test_gpu_unaligned.py, so that pytest has
generated the parametrised items of those two modules before this one appends to their list of cases (appended earlier, the
list would be longer than the `ids` those modules were given, and collection fails).

Known limit: tests/test_debug_fill.py requires every entry of every *SIGNATURES table of the bindings to be declared by a case
of that registry.  In a run that collects this file -- the whole suite, with or without -m gpu -- it is; tests/test_debug_fill.py
run in a process that never imports this file reports ma_normalize_local as neither exercised nor exempt."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _local_norm_ref as R  # noqa: E402
import test_gpu_stale_memory as S  # noqa: E402  (the registry: case, run_case, Env, dev)
import test_gpu_unaligned as U  # noqa: E402  (run_shifted)
from test_gpu_flow_smooth import taps_of  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPE = (67, 301)       # S.SHAPE: ragged against the tile, more than one block along x


def _case(name, dtype, r, kind, want, clip, min_support):
    @S.case(name, "ma_normalize_local")
    def make(env):
        ctx = env.ctx
        img = R.make_image(*SHAPE, dtype)
        weight = None if kind is None else R.make_weight(*SHAPE)[kind]
        taps, floor = taps_of(r), R.floor_of(dtype)
        e = R.normalize_local_ref(img, taps, floor, clip, weight, min_support)
        exp = ({n: e[n] for n in want}, e["counts"])

        def run():
            d_img, d_w = S.dev(ctx, img, weight)
            out, info = ctx.normalize_local(d_img, taps, floor, clip, d_w, min_support, want, return_info=True)
            alone = ctx.normalize_local(d_img, taps, floor, clip, d_w, min_support, want[:1])
            S.assert_same(alone[want[0]].numpy(), out[want[0]].numpy(), "one output alone, without the counts")
            return {n: out[n].numpy() for n in want}, tuple(info)
        return run, exp
    return make


_case("normalize_local[uint16, float weight, both outputs]", np.uint16, 7, 0, ("f32", "u8"), 2.0, 0.3)
_case("normalize_local[uint8, no weight, r=49]", np.uint8, 49, None, ("u8",), 4.0, 0.0)

CASES = [c for c in S.CASES if c.entries == ("ma_normalize_local",)]
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def env(ctx, tmp_path_factory):
    return S.Env(ctx, tmp_path_factory)


def test_the_cases_are_in_the_registry():
    assert len(CASES) == 2 and "ma_normalize_local" in S.declared_entries() and "ma_normalize_local" not in S.EXEMPT


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_call_on_stale_scratch_memory(ctx, env, monkeypatch, c):
    S.run_case(ctx, monkeypatch, env, c)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_call_at_shifted_addresses(ctx, env, monkeypatch, c):
    U.run_shifted(ctx, monkeypatch, env, c)


# ---- below the rule --------------------------------------------------------------------------------------------------------
# (parameter, dtype code of the image, weight kind, bytes of the element, what the pointer is moved by)
BELOW = [("img", 1, 0, 2, 1), ("img", 2, 0, 4, 1), ("img", 2, 0, 4, 2), ("weight", 0, 1, 4, 1), ("weight", 0, 1, 4, 2),
         ("out_f32", 0, 0, 4, 1), ("out_f32", 0, 0, 4, 2)]


@pytest.mark.parametrize("param,dtype,kind,nbytes,by", BELOW, ids=[f"{p}:{n}-byte element + {b}" for p, _, _, n, b in BELOW])
def test_a_pointer_below_the_rule_is_refused_before_any_launch(ctx, param, dtype, kind, nbytes, by):
    from microaligner_amd import _lib as L
    N = 8
    z = [ctx.zeros((16384,), F32) for _ in range(4)]
    sentinel = np.full(N * N, 7, F32)
    L.check(ctx.lib.ma_memcpy_h2d(ctx.handle, z[2].ptr, sentinel.ctypes.data, sentinel.nbytes))
    taps = (C.c_float * 2)(0.5, 0.25)
    counts = (C.c_longlong * 4)(-1, -1, -1, -1)
    good = dict(img=z[0].ptr, dtype=dtype, H=N, W=N, taps=taps, r=1, floor=1.0, clip=4.0, weight=z[1].ptr if kind else None,
                kind=kind, ms=0.0, out_f32=z[2].ptr, out_u8=z[3].ptr, counts=counts)
    bad = dict(good)
    bad[param] = good[param] + by
    rc = ctx.lib.ma_normalize_local(ctx.handle, *bad.values())
    msg = ctx.lib.ma_last_error().decode()
    assert rc == L.MA_EINVAL, (rc, msg)
    assert f"{param} must be {nbytes}-byte aligned" in msg, msg
    assert tuple(counts) == (-1, -1, -1, -1)
    ctx.sync()
    assert np.array_equal(z[2].numpy()[:N * N], sentinel)                # nothing was launched
    rc = ctx.lib.ma_normalize_local(ctx.handle, *good.values())
    assert rc == L.MA_OK, (rc, ctx.lib.ma_last_error().decode())
    # an all-zero image: every pixel is live, supported unless its weight is 0 (the all-zero weight), flat and 128
    assert tuple(counts) == ((N * N, 0, 0, 0) if kind else (0, 0, N * N, 0))
    assert (z[3].numpy().view(np.uint8)[:N * N] == 128).all() and not z[2].numpy()[:N * N].any()


@pytest.mark.parametrize("which", ["out_u8", "mask", "img"])
def test_a_uint8_array_has_no_address_below_the_rule(ctx, which):
    """at an odd address a uint8 image, mask or output is within the rule, and the result is the statement's"""
    from microaligner_amd import _lib as L
    img = R.make_image(*SHAPE, np.uint8)
    mask = R.make_weight(*SHAPE)[1]
    taps, floor = taps_of(7), R.floor_of(np.uint8)
    exp = R.normalize_local_ref(img, taps, floor, 4.0, mask, 0.05)
    alloc = U.Shifted(ctx, "edge", None, type(ctx).empty)
    d_img, d_mask, out = (alloc.view(SHAPE, np.uint8, 1 if which == n else 16) for n in ("img", "mask", "out_u8"))
    for d, a in ((d_img, img), (d_mask, mask)):
        L.check(ctx.lib.ma_memcpy_h2d(ctx.handle, d.ptr, a.ctypes.data, a.nbytes))
    counts = (C.c_longlong * 4)()
    ctx._run(ctx.lib.ma_normalize_local, d_img.ptr, L.MA_U8, *SHAPE, taps.ctypes.data_as(C.POINTER(C.c_float)), 7, floor, 4.0,
             d_mask.ptr, L.MA_SMOOTH_WEIGHT_U8, 0.05, None, out.ptr, counts)
    assert (d_img.ptr if which == "img" else d_mask.ptr if which == "mask" else out.ptr) % 2 == 1
    S.assert_same((out.numpy(), tuple(counts)), (exp["u8"], exp["counts"]), which)
    assert not alloc.slack_damage()
