"""-m gpu: one reader of the weight on the device (csrc/weight_map.h).  For each of the six calls that take a weight and every
kind it accepts, results that must be the same bits by the headers' definitions: a uint8 mask reads as 0 or 1, a weight of
1.0 multiplies exactly, a per-cell map is a lookup.  They differ if a reader, the dispatch of a kind or a MaWeight is wired
wrongly.  And the refusals of the weight argument at the six C entries.
(H, W) = (70, 130): one past the 64-line and two past the 128-output edge of both passes of the FIR tile, past the 32 x 64
tile of the median; cells (32, 50) are ragged in both axes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from microaligner_amd import _lib  # noqa: E402
from microaligner_amd.device import DeviceArray, gaussian_taps  # noqa: E402
from test_gpu_flow_invert import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
H, W, CELLS = 70, 130, (32, 50)
TAPS, FLOOR = gaussian_taps(1.0), 25.0
M = [[1.01, 0.02, -0.7], [-0.015, 0.99, 0.4]]


class Data:
    def __init__(self, ctx):
        rng = np.random.default_rng(7013)
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        img = 120 + 60 * np.cos(x / 5.0) * np.sin(y / 7.0) + rng.normal(0, 8, (H, W))
        self.flow = ctx.asdevice(rng.normal(0, 1.5, (H, W, 2)).astype(F32))
        self.ref = ctx.asdevice(np.clip(img, 0, 255).astype(np.uint8))
        self.img = ctx.asdevice((0.9 * img + 5 + rng.normal(0, 4, (H, W))).astype(F32))
        m = (rng.random((H, W)) >= 0.25).astype(np.uint8)
        c = rng.uniform(0.5, 2.0, (-(-H // CELLS[0]), -(-W // CELLS[1]))).astype(F32)
        c[1, 2] = 0.0
        self.mask = ctx.asdevice(m)                                                 # 0 / 1
        self.mask_any = ctx.asdevice(m * rng.integers(1, 256, (H, W)).astype(np.uint8))   # 0 / anything else
        self.mask_f32 = ctx.asdevice(m.astype(F32))
        self.ones = ctx.asdevice(np.ones((H, W), F32))
        self.cells = ctx.asdevice(c)
        self.cells_px = ctx.asdevice(np.ascontiguousarray(np.repeat(np.repeat(c, CELLS[0], 0), CELLS[1], 1)[:H, :W]))
        assert 0.15 < 1 - m.mean() < 0.35 and c.shape == (3, 3)


@pytest.fixture(scope="module")
def data(ctx):
    return Data(ctx)


def flat(res):
    """every array and every count of a result, as numpy arrays in a fixed order"""
    if isinstance(res, dict):
        return [a for k in sorted(res) for a in flat(res[k])]
    if isinstance(res, tuple):       # namedtuples of counts included
        return [a for v in res for a in flat(v)]
    return [res.numpy() if isinstance(res, DeviceArray) else np.asarray(res)]


def same(a, b):
    a, b = flat(a), flat(b)
    assert len(a) == len(b) and len(a) >= 2
    return all(same_bits(x, y) if x.dtype.kind == "f" else (x.dtype == y.dtype and np.array_equal(x, y)) for x, y in zip(a, b))


# name -> (call(ctx, data, weight, cell_size) -> every output, takes a per-cell map, the cell_size beside its expansion)
def smooth(where):
    return lambda ctx, d, w, cs: ctx.smooth_flow(d.flow, TAPS, w, cs, where=where, min_support=0.05, return_info=True)


def median(generic):
    return lambda ctx, d, w, cs: ctx.median_flow(d.flow, 2, w, cs, where="outliers", thresh=0.75, return_info=True, keep=True,
                                                 generic=generic)


CALLS = {
    "smooth_all": (smooth("all"), True, None),
    "smooth_blend": (smooth("blend"), True, None),
    "median_registers": (median(False), True, None),
    "median_generic": (median(True), True, None),
    "affine_moments": (lambda ctx, d, w, cs: ctx.flow_affine_moments(d.flow, w, CELLS), True, CELLS),
    "affine_moments_trimmed": (lambda ctx, d, w, cs: ctx.flow_affine_moments(d.flow, w, CELLS, prior=[[1, 0, 0], [0, 1, 0]],
                                                                              clip=2.0), True, CELLS),
    "direct_affine": (lambda ctx, d, w, cs: ctx.direct_affine_moments(d.ref, d.img, M, 1.1, -4.0, w, clip=40.0), False, None),
    "refine_step": (lambda ctx, d, w, cs: ctx.flow_refine_step(d.ref, d.img, d.flow, TAPS, FLOOR, w, return_info=True),
                    False, None),
    "local_correlation": (lambda ctx, d, w, cs: ctx.local_correlation(d.ref, d.img, TAPS, FLOOR, (120.0, 113.0), w,
                                                                      cell_size=CELLS, want=("score", "weight")), False, None),
}


@pytest.mark.parametrize("name", CALLS)
def test_the_kinds_of_a_weight_agree(ctx, data, name):
    call, per_cell, cs_px = CALLS[name]
    with_f32 = call(ctx, data, data.mask_f32, None)
    assert same(call(ctx, data, data.mask, None), with_f32), "a uint8 mask against the same weights in float32"
    assert same(call(ctx, data, data.mask_any, None), with_f32), "a mask is nonzero or zero"
    plain = call(ctx, data, None, None)
    assert same(plain, call(ctx, data, data.ones, None)), "no weight against a weight of 1.0"
    assert not same(plain, with_f32), "the weight is read at all"
    if per_cell:
        assert same(call(ctx, data, data.cells, CELLS), call(ctx, data, data.cells_px, cs_px)), \
            "a per-cell map against its expansion to pixels"


# ---- refusals of the weight argument at the C entries --------------------------------------------------------------------------
def test_the_c_entries_refuse_a_bad_weight(ctx, data):
    d = data
    taps, r = TAPS.ctypes.data_as(C.POINTER(C.c_float)), len(TAPS) - 1
    out = ctx.asdevice(np.full((H, W, 2), 7, F32))
    keep = ctx.asdevice(np.full((H, W), 7, np.uint8))
    plane = [ctx.asdevice(np.full((H, W), 7, F32)) for _ in range(2)]
    sums = np.full(3 * 3 * _lib.MA_FLOW_AFFINE_SUMS + _lib.MA_DIRECT_AFFINE_SUMS, 7.0)
    counts = np.full(64, 7, np.int64)
    p_sums, p_counts = sums.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_longlong))
    m = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    lib, NONE, PIXELS, MASK, PER_CELL = ctx.lib, 0, 1, 2, 3
    assert (NONE, PIXELS, MASK, PER_CELL) == (_lib.MA_SMOOTH_WEIGHT_NONE, _lib.MA_SMOOTH_WEIGHT_F32, _lib.MA_SMOOTH_WEIGHT_U8,
                                              _lib.MA_SMOOTH_WEIGHT_CELLS)
    # name -> (entry(weight, kind) -> return code, takes a per-cell map)
    entries = {
        "smooth": (lambda w, k: lib.ma_smooth_flow(ctx.handle, d.flow.ptr, H, W, taps, r, w, k, *CELLS, _lib.MA_SMOOTH_ALL, 0.0,
                                                   out.ptr, p_counts), True),
        "median": (lambda w, k: lib.ma_median_flow(ctx.handle, d.flow.ptr, H, W, 2, w, k, *CELLS, _lib.MA_MEDIAN_ALL, 1.0, 0,
                                                   out.ptr, keep.ptr, p_counts), True),
        "affine": (lambda w, k: lib.ma_flow_affine_moments(ctx.handle, d.flow.ptr, H, W, w, k, *CELLS, None, 0.0, p_sums,
                                                           p_counts), True),
        "direct": (lambda w, k: lib.ma_direct_affine_moments(ctx.handle, d.ref.ptr, _lib.MA_U8, d.img.ptr, _lib.MA_F32, H, W, m,
                                                             1.0, 0.0, w, k, 0.0, p_sums, p_counts), False),
        "refine": (lambda w, k: lib.ma_flow_refine_step(ctx.handle, d.ref.ptr, _lib.MA_U8, d.img.ptr, H, W, taps, r, FLOOR, w, k,
                                                        1.0, d.flow.ptr, out.ptr, p_counts), False),
        "localcorr": (lambda w, k: lib.ma_local_correlation(ctx.handle, d.ref.ptr, _lib.MA_U8, d.img.ptr, H, W, taps, r, 0.0, 0.0,
                                                            FLOOR, w, k, 0.0, 0.25, 0.75, plane[0].ptr, plane[1].ptr, *CELLS,
                                                            p_counts), False),
    }
    for name, (entry, per_cell) in entries.items():
        bad = [(d.ones.ptr, 4), (d.ones.ptr, -1), (None, PIXELS), (None, MASK), (None, PER_CELL)]
        if not per_cell:
            bad.append((d.cells.ptr, PER_CELL))
        for w, k in bad:
            assert entry(w, k) == _lib.MA_EINVAL, (name, w is None, k)
    ctx.sync()
    # nothing was launched: no output of any entry was written
    assert (sums == 7.0).all() and (counts == 7).all() and (keep.numpy() == 7).all()
    assert all((a.numpy() == 7).all() for a in [out] + plane)
    # and each entry takes what it accepts
    for name, (entry, per_cell) in entries.items():
        good = [(None, NONE), (d.ones.ptr, NONE), (d.ones.ptr, PIXELS), (d.mask.ptr, MASK)] + ([(d.cells.ptr, PER_CELL)] * per_cell)
        for w, k in good:
            assert entry(w, k) == _lib.MA_OK, (name, k)
    ctx.sync()
