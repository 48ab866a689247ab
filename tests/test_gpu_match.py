"""-m gpu: ma_match_similarity (csrc/ransac.hip: ratio test, ordered compaction, two-instalment sample scoring, refinement) on the
cases of tests/test_match_ref.py, which proves on the CPU that the cases reach the paths they are named after and that their
expectations are the project's definition.  One device call per case, compared with tests/_match_ref.py:match_ref alone --
never with another device call: the same number of good matches, the same status, the same matrix bits (np.array_equal)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _match_ref as MR  # noqa: E402
import test_match_ref as R  # noqa: E402
from microaligner_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


def _call(ctx, c, **kw):
    p = dict(n_train=None if c.n_train == len(c.tpts) else c.n_train, **c.params)
    p["reproj_threshold"] = p.pop("thr")
    p.update(kw)
    return ctx.match_similarity(ctx._upload_raw(c.idx), ctx._upload_raw(c.dist_sq), ctx._upload_raw(c.qpts),
                                ctx._upload_raw(c.tpts), **p)


def _same(got, exp, what):
    mat, n_good, status = got
    emat, en_good, estatus = exp[:3]
    assert (n_good, status) == (en_good, estatus), (what, n_good, status, en_good, estatus)
    if emat is None:
        assert mat is None, what
    else:
        assert mat is not None and np.array_equal(mat, emat), (what, mat, emat)


def _check(ctx, name):
    c = R.BY_NAME[name]
    _same(_call(ctx, c), R.expected(c), name)


@pytest.mark.parametrize("name", R.NAMES)
def test_device_equals_the_reference(ctx, name):
    _check(ctx, name)


def test_state_across_calls(ctx):
    """A call that runs both instalments, two early returns (too few matches; coordinates refused) and the first call again:
    the same bits.  Then max_iters = 1 followed by max_iters = 2000, which grows the page-locked scratch between two calls."""
    first = _call(ctx, R.BY_NAME["second_instalment"])
    _same(first, R.expected(R.BY_NAME["second_instalment"]), "second_instalment")
    for name in ("n_good_1", "large_refused_n64"):
        _check(ctx, name)
    again = _call(ctx, R.BY_NAME["second_instalment"])
    _same(again, R.expected(R.BY_NAME["second_instalment"]), "second_instalment, again")
    assert first[1:] == again[1:] and first[0].tobytes() == again[0].tobytes()
    for name in ("max_iters_1", "second_instalment", "single_block_passes_nq3100_max_iters_1_noisy", "nq_3100_noisy"):
        _check(ctx, name)


def test_bad_arguments_are_refused_by_the_c_entry(ctx):
    """MA_EINVAL for empty sizes, max_iters outside [1, 1000000], confidence outside (0, 1), a threshold of 0 and every NULL
    pointer the entry names; nothing is written, and a valid call afterwards gives the reference's bits."""
    c = R.BY_NAME["nq_65_noisy"]
    bufs = [ctx._upload_raw(a) for a in (c.idx, c.dist_sq, c.qpts, c.tpts)]
    mat = (C.c_double * 6)(*[7.0] * 6)
    n_good, status = C.c_int(-5), C.c_int(-5)
    ok = dict(idx=bufs[0].ptr, dist=bufs[1].ptr, nq=len(c.idx), qpts=bufs[2].ptr, tpts=bufs[3].ptr, nt=len(c.tpts), ratio=c.ratio,
              confidence=c.confidence, thr=c.thr, max_iters=c.max_iters, rng=None, mat=mat, n_good=C.byref(n_good),
              status=C.byref(status))
    call = lambda **kw: ctx.lib.ma_match_similarity(ctx.handle, *dict(ok, **kw).values())     # noqa: E731
    for kw in (dict(nq=0), dict(nq=-1), dict(nt=0), dict(nt=-1), dict(max_iters=0), dict(max_iters=-1), dict(max_iters=1000001),
               dict(confidence=0.0), dict(confidence=1.0), dict(confidence=-0.5), dict(confidence=1.5),
               dict(confidence=float("nan")), dict(thr=0.0), dict(thr=-3.0), dict(thr=float("nan")),
               dict(idx=None), dict(dist=None), dict(qpts=None), dict(tpts=None), dict(mat=None), dict(n_good=None),
               dict(status=None)):
        assert call(**kw) == _lib.MA_EINVAL, kw
    assert ctx.lib.ma_match_similarity(None, *ok.values()) == _lib.MA_EINVAL
    assert list(mat) == [7.0] * 6 and (n_good.value, status.value) == (-5, -5)          # a refused call wrote nothing
    # rng_state NULL is numpy's seed 0, the case's seed
    assert c.seed == 0 and call() == _lib.MA_OK
    emat, en_good, estatus, _ = R.expected(c)
    assert (n_good.value, status.value) == (en_good, estatus) and estatus == 0
    assert np.array_equal(np.array(mat).reshape(2, 3), emat)
    _check(ctx, "nq_65_noisy")


def test_n_train_bounds_the_first_neighbour(ctx):
    """A train buffer of 400 points of which 300 count (device-made features keep their points in a buffer of capacity size):
    good matches whose first neighbour is 300, 399 or -1 are not counted and the rest keep their order -- match_ref with
    n_train = 300.  Without n_train the buffer's size is the bound (the behaviour before the argument existed): the matches
    at 300 and 399 count.  Every index stays inside the allocation, whatever the guard does."""
    rng = np.random.default_rng(20)
    nq, n_train, cap = 300, 300, 400
    src, dst = R.noisy_pairs(rng, nq, 0.6, 1.2)
    idx, dist_sq, qpts, tpts = R.embed(rng, src, dst, nq, np.arange(nq), decoys=0)
    tpts = np.concatenate([tpts, rng.integers(0, 1500, (cap - n_train, 2)).astype(np.float64)])     # integer-valued, too
    outside = np.array([0, 63, 64, 150, 299])
    idx[outside, 0] = [300, 399, -1, 399, 300]
    args = (np.ascontiguousarray(idx, np.int32), dist_sq, qpts, tpts)
    dev = [ctx._upload_raw(a) for a in args]
    exp = MR.match_ref(*args, n_train)
    good = exp[3]["good"]
    assert not good[outside].any() and good.sum() == exp[1] == nq - len(outside) and exp[2] == 0
    _same(ctx.match_similarity(*dev, n_train=n_train), exp, "n_train = 300")
    exp_cap = MR.match_ref(*args, cap)
    assert exp_cap[1] == nq - 1 and exp_cap[2] == 0 and not np.array_equal(exp_cap[0], exp[0])
    _same(ctx.match_similarity(*dev), exp_cap, "n_train = None")
    _same(ctx.match_similarity(*dev, n_train=cap), exp_cap, "n_train = 400")
    with pytest.raises(ValueError):
        ctx.match_similarity(*dev, n_train=cap + 1)
