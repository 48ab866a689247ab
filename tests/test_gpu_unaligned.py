"""-m gpu: every device call at unaligned device addresses.

Context.empty rounds an allocation up to 64 KiB and hands out its base, so every pointer the rest of the suite passes to a C
entry is aligned to 64 KiB.  The C ABI takes any device pointer within the rule of include/microaligner_hip.h ("Device
pointers"): aligned to its element; an array of pairs (flows, maps, grid nodes, points) to the pair; stricter only where a
header names an argument.  Within the rule every result is the same as at an aligned address; below it an entry returns
MA_EINVAL before it launches anything.

The first half runs the registry of tests/_gpu_cases, as tests/test_gpu_stale_memory.py does.  Every case builds its inputs
and its expected result once and runs its call three times: with the plain allocator, and twice with Context.empty replaced
by one that allocates 64 bytes more, fills the whole allocation with 0xFF and hands out a view at an offset inside it
(Context._upload_raw likewise, by the shape and type of the array it uploads; Context._raw, whose untyped bytes a call fills
with int32, float64 or pairs of float64, by the strictest of those) --

  edge : the address is = A (mod 16) for an array whose alignment under the rule is A <= 8, = 16 (mod 32) for A = 16,
         = 32 (mod 64) for A = 32: as far off every larger boundary as the rule allows;
  half : the address is = 8 (mod 16) for every array with A <= 8 (the arms that are "8-byte but not 16-byte aligned":
         flow_affine.hip, qc.hip, pyramid.hip), the edge address otherwise.

Each shifted result must satisfy the case's statement exactly as in the stale-memory test, and be bit-identical to the
plain run (BIT_EXEMPT names what is not, and why).  Context._run is wrapped: a pointer argument that falls inside a shifted
allocation must lie inside the view, never in the slack; every C entry the case declares must have been called and must have
received the pointer of a view; one of them off every 16-byte boundary unless ALIGNED16 says why it cannot.  After the pass the
0xFF in front of and behind every view must still be there.

One direct test follows: pyr_down at a width of its vector arm, the only fast arm that the shape can switch off before the
address is looked at.

The second half calls every checked entry below the rule: REJECT lists (entry, parameter, bytes) for every pointer argument
that a kernel reads or writes through a wider type than it is declared with (MA_REQUIRE_ALIGNED in the sources); CALLS holds
valid arguments of a small legal size for each entry.  With that one pointer bytes / 2 past an aligned address the entry must
return MA_EINVAL and name the parameter in ma_last_error(); the same call with the pointer put back must succeed, which it
would not after a launch on a misaligned record or with a profile scope left open.  Where an entry checks an argument against
the size of its element (ELEMENT_SIZED: ma_normalize_local), BELOW lists the pointers below that, and a uint8 array is shown
to have no such address.

tests/test_unaligned_tables.py (no GPU) checks offset_for and holds REJECT, CALLS, OVERRIDES, BELOW and ELEMENT_SIZED against
the headers and the sources.

Observed on an MI355X: all 89 cases give the bits of the plain run at both sets of addresses, the float64 sums of
ma_flow_affine_moments apart.  With joint_hist16_kernel's scalar loop made wrong where its vector arm is switched off
(`count(a[i], b[i + (vec_ok ? 0 : 1)])`, nmi.hip) the two nmi_scores cases and the two feature_round cases of this file fail,
against the statement and against the plain run, while the same cases of tests/test_gpu_stale_memory.py pass: they never leave
the vector arm.  The file takes 7.7 s where the stale-memory file takes 8.8 s (89 cases each, the second half included)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytest.register_assert_rewrite("_gpu_cases")       # the cases' own asserts are quoted by run_shifted: keep them informative
import _gpu_cases as G  # noqa: E402  (the registry: CASES, Env, assert_same)
from _gpu_cases.dog import _DT  # noqa: E402
from _gpu_cases.pyramid import _image  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SLACK = 64
PASSES = ("edge", "half")

# Arguments whose header states more than the general rule, by case: what the shifted allocator aligns to instead.
# "f64": every float64 array (and the untyped buffers that hold them); "pair": every array of pairs.  Each entry quotes its
# header sentence; the table holds nothing else.
OVERRIDES = {
    "landmark_flow, landmark_points": (
        {"f64": 32}, "include/microaligner_landmarks.h: \"cw: n x 4 doubles on the device, 32-byte aligned\""),
    "pyr_up_flow": (
        {"pair": 16}, "include/microaligner_hip.h, ma_pyr_up_flow: \"dst must be 16-byte aligned (it is written two pixels at "
                      "a time)\""),
    "optflow_register[companion stream on]": (
        {"pair": 16}, "include/microaligner_hip.h, ma_optflow_register: \"flow_out must be 16-byte aligned: it is the dst of "
                      "the ma_pyr_up_flow that ends the call\""),
    "optflow_register[companion stream off]": (
        {"pair": 16}, "include/microaligner_hip.h, ma_optflow_register: \"flow_out must be 16-byte aligned: it is the dst of "
                      "the ma_pyr_up_flow that ends the call\""),
}

# Cases whose shifted result is not compared bit for bit with the plain run, and the part that still is: each names the
# floating-point reduction whose order of summation follows the load width.
BIT_EXEMPT = {
    "flow_affine_moments, flow_affine_apply": (
        "fa_moments_kernel adds a lane's two pixels of a 16-byte load to its float64 sums where the flow is 16-byte aligned "
        "and one pixel per lane where it is only 8-byte aligned (flow_affine.hip, vec_ok): the 14 sums of a cell are added in "
        "another order, within the bound the statement checks; the counts and flow_affine_apply compare exactly",
        lambda res: ([counts for _, counts in res[0]], res[1])),
}

# Declared entries that cannot receive a pointer off every 16-byte boundary: every device array they take is held to 16
# bytes or more by the rule or by OVERRIDES.
ALIGNED16 = {
    "ma_landmark_points": "cw at 32 bytes (OVERRIDES), pts and out pairs of float64 at 16",
    "ma_pyr_up_flow": "dst at 16 bytes (OVERRIDES); src is a flow of the same case and moves with it",
}


def alignment_of(shape, dtype, override=None):
    """A: the alignment of an array under the rule -- the pair where the last of two or more axes has length 2, else the
    element -- or what `override` states for its kind, if that is more"""
    dtype = np.dtype(dtype)
    pair = len(shape) >= 2 and shape[-1] == 2
    a = dtype.itemsize * (2 if pair else 1)
    if override:
        if pair and "pair" in override:
            a = max(a, override["pair"])
        if dtype == np.float64 and "f64" in override:
            a = max(a, override["f64"])
    return a


def offset_for(shape, dtype, which, override=None):
    """the byte offset of a view from a base that is aligned to 64 bytes, so that the view's address has the residue of
    the pass `which` (module docstring)"""
    a = alignment_of(shape, dtype, override)
    assert a in (1, 2, 4, 8, 16, 32), a
    if which == "half" and a <= 8:
        return 8
    assert which in PASSES, which
    return a            # A (mod 16) for A <= 8, 16 (mod 32), 32 (mod 64)


def raw_alignment(override=None):
    """Context._raw hands out untyped bytes that its callers fill with int32, float64 or pairs of float64: the strictest of
    those under the rule, or what `override` states"""
    return max([16] + list((override or {}).values()))


class Shifted:
    """the allocator of one pass of one case, and what it handed out"""

    def __init__(self, ctx, which, override, plain_empty):
        self.ctx, self.which, self.override, self.plain_empty = ctx, which, override, plain_empty
        self.bases, self.views = [], []         # views: (address, bytes, base address)

    def view(self, shape, dtype, off):
        from microaligner_amd import _lib as L
        from microaligner_amd.device import DeviceArray
        shape, dtype = tuple(int(s) for s in shape), np.dtype(dtype)
        nbytes = max(int(np.prod(shape, dtype=np.int64)) * dtype.itemsize, 1)
        base = self.plain_empty(self.ctx, (nbytes + SLACK,), np.uint8)
        assert base.ptr % SLACK == 0 and 0 < off < SLACK and (base.ptr + off) % dtype.itemsize == 0
        L.check(self.ctx.lib.ma_memset(self.ctx.handle, base.ptr, 0xFF, nbytes + SLACK))
        self.bases.append(base)
        self.views.append((base.ptr + off, nbytes, base.ptr))
        return DeviceArray(self.ctx, shape, dtype, base.ptr + off, 0, owner=False)

    def empty(self, shape, dtype):
        return self.view(shape, dtype, offset_for(tuple(int(s) for s in shape), dtype, self.which, self.override))

    def raw(self, nbytes):
        a = raw_alignment(self.override)
        return self.view((max(int(nbytes), 1),), np.uint8, a)

    def upload_raw(self, arr):
        """Context._upload_raw, the untyped buffer placed by what it holds"""
        from microaligner_amd import _lib as L
        arr = np.ascontiguousarray(arr)
        buf = self.view((max(arr.nbytes, 1),), np.uint8, offset_for(arr.shape, arr.dtype, self.which, self.override))
        if arr.nbytes:
            L.check(self.ctx.lib.ma_memcpy_h2d(self.ctx.handle, buf.ptr, arr.ctypes.data, arr.nbytes))
        return buf

    def slack_damage(self):
        """the views whose 0xFF in front or behind is no longer there"""
        from microaligner_amd import _lib as L
        bad = []
        host = np.zeros(SLACK, np.uint8)
        for ptr, nbytes, base in self.views:
            front, back = ptr - base, SLACK - (ptr - base)
            for name, at, n in (("in front of", base, front), ("behind", ptr + nbytes, back)):
                host[:] = 0
                L.check(self.ctx.lib.ma_memcpy_d2h(self.ctx.handle, host.ctypes.data, at, n))
                if not (host[:n] == 0xFF).all():
                    bad.append(f"{name} the {nbytes} bytes at base + {front}: {host[:n].tolist()}")
        return bad


def pointer_values(args):
    """the integer and pointer arguments of a call as addresses"""
    out = []
    for a in args:
        if isinstance(a, bool):
            continue
        if isinstance(a, (int, np.integer)):
            out.append(int(a))
        elif isinstance(a, C.c_void_p) and a.value:
            out.append(int(a.value))
    return out


def run_shifted(ctx, monkeypatch, env, c):
    from microaligner_amd.device import Context
    plain_run, plain_empty, plain_raw, plain_upload = Context._run, Context.empty, Context._raw, Context._upload_raw
    override = OVERRIDES.get(c.name, (None, ""))[0]
    state = {"alloc": None, "called": {}}       # called: entry -> the addresses of views it received, per pass

    def recording_run(self, fn, *args):
        got = state["called"].setdefault(fn.__name__, [])
        alloc = state["alloc"]
        if alloc is not None:
            for p in pointer_values(args):
                for ptr, nbytes, base in alloc.views:
                    if base <= p < base + nbytes + SLACK:
                        assert ptr <= p < ptr + nbytes, \
                            f"{fn.__name__} received {p - base} bytes into an allocation whose view is at {ptr - base}: the slack"
                        if p == ptr:
                            got.append(p)
        return plain_run(self, fn, *args)

    monkeypatch.setattr(Context, "_run", recording_run)
    env.poison = 0xFF
    ctx._resident.clear()
    run, expected = c.make(env)
    results, failed = [run()], []
    ctx.sync()
    ctx._resident.clear()
    for which in PASSES:
        alloc = Shifted(ctx, which, override, plain_empty)
        state["alloc"], state["called"] = alloc, {}
        monkeypatch.setattr(Context, "empty", lambda self, shape, dtype, a=alloc: a.empty(shape, dtype))
        monkeypatch.setattr(Context, "_raw", lambda self, nbytes, a=alloc: a.raw(nbytes))
        monkeypatch.setattr(Context, "_upload_raw", lambda self, arr, a=alloc: a.upload_raw(arr))
        try:
            results.append(run())
            ctx.sync()
        finally:
            monkeypatch.setattr(Context, "empty", plain_empty)
            monkeypatch.setattr(Context, "_raw", plain_raw)
            monkeypatch.setattr(Context, "_upload_raw", plain_upload)
            state["alloc"] = None
            ctx._resident.clear()       # no view outlives the allocations behind it
        failed += [f"{which}: the 0xFF {b} was overwritten" for b in alloc.slack_damage()]
        if not alloc.views:
            failed.append(f"{which}: the shifted allocator handed out no array")
        for e in c.entries:
            seen = state["called"].get(e)
            if seen is None:
                failed.append(f"{which}: declared but never called: {e}")
            elif not seen:
                failed.append(f"{which}: {e} received no pointer of a shifted array")
            elif e not in ALIGNED16 and all(p % 16 == 0 for p in seen):
                failed.append(f"{which}: every shifted pointer {e} received is 16-byte aligned")
        alloc.bases.clear()
    for k, res in enumerate(results):
        name = ("plain",) + PASSES
        try:
            if callable(expected):
                expected(res)
            else:
                G.assert_same(res, expected, name[k])
        except AssertionError as e:
            failed.append(f"{name[k]}: against the statement: {str(e).splitlines()[0] if str(e) else repr(e)}")
        if c.bits and k:
            part = BIT_EXEMPT[c.name][1] if c.name in BIT_EXEMPT else (lambda r: r)
            try:
                G.assert_same(part(res), part(results[0]), name[k])
            except AssertionError as e:
                failed.append(f"{name[k]}: against the plain run: {str(e).splitlines()[0] if str(e) else repr(e)}")
    assert not failed, f"{len(failed)} checks failed:\n" + "\n".join(failed)


@pytest.fixture(scope="module")
def env(ctx, tmp_path_factory):
    return G.Env(ctx, tmp_path_factory)


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_call_at_shifted_addresses(ctx, env, monkeypatch, c):
    run_shifted(ctx, monkeypatch, env, c)


def test_the_tables_name_cases_and_entries_of_the_registry():
    names = {c.name for c in G.CASES}
    assert set(OVERRIDES) <= names and set(BIT_EXEMPT) <= names
    assert set(ALIGNED16) <= G.declared_entries()
    for table in (OVERRIDES, BIT_EXEMPT):
        for key, (_, *rest) in table.items():
            assert all(rest), key
    for c in G.CASES:
        if c.name in BIT_EXEMPT:
            assert c.bits, c.name
    assert all(isinstance(r, str) and r.strip() for r in ALIGNED16.values())


# ---- the one arm the registry does not choose by the address --------------------------------------------------------------
# Every other fast arm is chosen from the address bits alone (nmi.hip, qc.hip, dog.hip, quantile.hip, flow_affine.hip), so
# the shifted registry takes the fall-back of each.  pyr_down's is chosen by `w % 4 == 0 && src % 16 == 0 && dst % 8 == 0`
# (pyramid.hip), and every width of the registry is odd: the address terms decide nothing there.  Here w % 4 == 0, more than
# one block along x, and either src or dst is one element past a 16-byte boundary.
@pytest.mark.parametrize("moved", ("src", "dst", "both"))
@pytest.mark.parametrize("dtype", (np.uint8, np.uint16, np.float32), ids=lambda d: np.dtype(d).name)
def test_pyr_down_with_a_width_of_the_vector_arm_at_an_element_aligned_address(ctx, dtype, moved):
    from microaligner_amd.device import Context
    h, w = 64, 2052
    img = _image((h, w), dtype, 71)
    exp = G._O().pyr_down(img)
    ctx._resident.clear()
    plain = ctx.pyr_down(ctx.asdevice(img)).numpy()
    G.assert_same(plain, exp, "at aligned addresses")
    size = np.dtype(dtype).itemsize
    alloc = Shifted(ctx, "edge", None, Context.empty)
    src = alloc.view((h, w), dtype, size if moved != "dst" else 16)
    dst = alloc.view(exp.shape, dtype, size if moved != "src" else 16)
    from microaligner_amd import _lib as L
    L.check(ctx.lib.ma_memcpy_h2d(ctx.handle, src.ptr, img.ctypes.data, img.nbytes))
    ctx._run(ctx.lib.ma_pyr_down, src.ptr, _DT[np.dtype(dtype)], h, w, dst.ptr)
    got = dst.numpy()
    ctx._resident.clear()
    G.assert_same(got, exp, f"{moved} moved by {size}")
    assert not alloc.slack_damage()


# ---- below the rule -------------------------------------------------------------------------------------------------------
# (entry, parameter, bytes, position of the parameter in the C prototype, ctx being 0): every pointer argument that a kernel
# reads or writes through a wider type than it is declared with.  The last four rows' checks are older than the helper.
REJECT = [
    ("ma_farneback_tiled", "flow_out", 8, 13),
    ("ma_farneback_levels", "flow_out", 8, 13),
    ("ma_farneback_debug", "flow_out", 8, 10),
    ("ma_optflow_register", "flow_out", 16, 7),
    ("ma_remap_bilinear", "map_xy", 8, 6),
    ("ma_remap_interp", "map_xy", 8, 6),
    ("ma_warp_tiled", "flow", 8, 5),
    ("ma_warp_tiled_minmax", "flow", 8, 5),
    ("ma_warp_tiled_flowcells", "flow", 8, 5),
    ("ma_warp_tiled_interp", "flow", 8, 5),
    ("ma_warp_pages_host", "flow", 8, 7),
    ("ma_warp_pages_host_interp", "flow", 8, 7),
    ("ma_merge_flows_tiled", "flow1", 8, 1),
    ("ma_merge_flows_tiled", "flow2", 8, 2),
    ("ma_merge_flows_tiled", "out", 8, 7),
    ("ma_merge_flows_tiled_cells", "flow1", 8, 1),
    ("ma_merge_flows_tiled_cells", "flow2", 8, 2),
    ("ma_merge_flows_tiled_cells", "out", 8, 9),
    ("ma_warp_affine_flow", "flow", 8, 7),
    ("ma_warp_affine_flow_pages_host", "flow", 8, 9),
    ("ma_warp_affine_grid", "nodes", 8, 7),
    ("ma_warp_affine_grid_pages_host", "nodes", 8, 9),
    ("ma_compose_flows", "first", 8, 1),
    ("ma_compose_flows", "second", 8, 2),
    ("ma_compose_flows", "out", 8, 5),
    ("ma_invert_flow", "flow", 8, 1),
    ("ma_invert_flow", "out", 8, 6),
    ("ma_transform_points", "pts", 16, 1),
    ("ma_transform_points", "flow", 8, 3),
    ("ma_transform_points", "out", 16, 13),
    ("ma_transform_points_grid", "pts", 16, 1),
    ("ma_transform_points_grid", "nodes", 8, 3),
    ("ma_transform_points_grid", "out", 16, 14),
    ("ma_flow_grid_sample", "flow", 8, 1),
    ("ma_flow_grid_sample", "nodes", 8, 5),
    ("ma_flow_grid_expand", "nodes", 8, 1),
    ("ma_flow_grid_expand", "out", 8, 5),
    ("ma_flow_grid_error", "flow", 8, 1),
    ("ma_flow_grid_error", "nodes", 8, 2),
    ("ma_smooth_flow", "flow", 8, 1),
    ("ma_smooth_flow", "out", 8, 12),
    ("ma_flow_fold_mask", "flow", 8, 1),
    ("ma_median_flow", "flow", 8, 1),
    ("ma_median_flow", "out", 8, 12),
    ("ma_fill_flow", "flow", 8, 1),
    ("ma_fill_flow", "out", 8, 8),
    ("ma_flow_refine_step", "flow", 8, 12),
    ("ma_flow_refine_step", "out", 8, 13),
    ("ma_flow_affine_apply", "flow", 8, 1),
    ("ma_flow_affine_apply", "out", 8, 5),
    ("ma_landmark_flow", "out", 8, 10),
    ("ma_landmark_points", "pts", 16, 7),
    ("ma_landmark_points", "out", 16, 9),
    ("ma_pyr_up_flow", "src", 8, 1),
    # checked before this helper existed
    ("ma_flow_affine_moments", "flow", 8, 1),
    ("ma_qc_flow_grid", "flow", 8, 1),
    ("ma_landmark_flow", "cw", 32, 1),
    ("ma_landmark_points", "cw", 32, 1),
    ("ma_pyr_up_flow", "dst", 16, 5),
]

N = 8           # the side of the flows and images of the calls below; Farneback and the registration take larger ones
FB = 16
REG = (131, 157)


class Bufs:
    """device and host memory for the calls of CALLS: six zeroed 64 KiB device buffers (an all-zero flow, map, grid, image or
    list of points is a valid one), host matrices, taps and result arrays, two host pages, and a pair of images with a flow
    for the registration"""

    def __init__(self, ctx):
        self.z = [ctx.zeros((16384,), F32) for _ in range(6)]
        self.p = [a.ptr for a in self.z]
        self.m6 = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
        self.taps = (C.c_float * 2)(0.5, 0.25)
        self.page, self.page_out = np.zeros((N, N), np.uint8), np.zeros((N, N), np.uint8)
        self.pages, self.outs = (C.c_void_p * 1)(self.page.ctypes.data), (C.c_void_p * 1)(self.page_out.ctypes.data)
        self.d, self.ll, self.ll2, self.f = (C.c_double * 16)(), (C.c_longlong * 16)(), (C.c_longlong * 16)(), (C.c_float * 16)()
        self.d2, self.d3 = (C.c_double * 16)(), (C.c_double * 16)()
        ref, mov = G.pair(*REG, seed=1)
        self.ref, self.mov = ctx.asdevice(ref), ctx.asdevice(mov)
        self.reg_flow = ctx.empty(REG + (2,), F32)
        from microaligner_amd import _lib as L
        self.params = L.MaParams(1, 3, 60, 10, 1, 0, 0, 0)
        self.reports, self.n_reports = (L.MaLevelReport * 4)(), C.c_int(0)


# entry -> the arguments after ctx of a valid call, b being the Bufs
CALLS = {
    "ma_farneback_tiled": lambda b: [b.p[0], b.p[1], 2, FB, FB, 0, 0, 5, 1, 1, 1.7, 0, b.p[2]],
    "ma_farneback_levels": lambda b: [b.p[0], b.p[1], 2, FB, FB, 0, 0.5, 5, 1, 1, 1.7, 0, b.p[2]],
    "ma_farneback_debug": lambda b: [b.p[0], b.p[1], 2, FB, FB, 5, 1, 1.7, 0, b.p[2], b.p[3], b.p[4], b.p[5]],
    "ma_optflow_register": lambda b: [b.ref.ptr, b.mov.ptr, 2, REG[0], REG[1], C.byref(b.params), b.reg_flow.ptr, b.reports, 4,
                                      C.byref(b.n_reports)],
    "ma_remap_bilinear": lambda b: [b.p[0], 0, 1, N, N, b.p[1], N, N, b.p[2]],
    "ma_remap_interp": lambda b: [b.p[0], 0, 1, N, N, b.p[1], N, N, b.p[2], 2],
    "ma_warp_tiled": lambda b: [b.p[0], 0, N, N, b.p[1], 0, 0, b.p[2]],
    "ma_warp_tiled_minmax": lambda b: [b.p[0], 0, N, N, b.p[1], 0, 0, b.p[2], b.p[3]],
    "ma_warp_tiled_flowcells": lambda b: [b.p[0], 0, N, N, b.p[1], 4, 1, b.p[2], b.p[3], b.p[4]],
    "ma_warp_tiled_interp": lambda b: [b.p[0], 0, N, N, b.p[1], 0, 0, b.p[2], 2],
    "ma_warp_pages_host": lambda b: [b.pages, b.outs, 1, 0, N, N, b.p[1], 0, 0],
    "ma_warp_pages_host_interp": lambda b: [b.pages, b.outs, 1, 0, N, N, b.p[1], 0, 0, 2],
    "ma_merge_flows_tiled": lambda b: [b.p[0], b.p[1], N, N, 0, 0, b.p[2]],
    "ma_merge_flows_tiled_cells": lambda b: [b.p[0], b.p[1], N, N, 4, 1, b.p[3], b.p[4], b.p[2]],
    "ma_warp_affine_flow": lambda b: [b.p[0], 0, N, N, 0, 0, b.p[1], N, N, b.m6, b.p[2], 1],
    "ma_warp_affine_flow_pages_host": lambda b: [b.pages, b.outs, 1, 0, N, N, 0, 0, b.p[1], N, N, b.m6, 1],
    "ma_warp_affine_grid": lambda b: [b.p[0], 0, N, N, 0, 0, b.p[1], N, N, 4, b.m6, b.p[2], 1],
    "ma_warp_affine_grid_pages_host": lambda b: [b.pages, b.outs, 1, 0, N, N, 0, 0, b.p[1], N, N, 4, b.m6, 1],
    "ma_compose_flows": lambda b: [b.p[0], b.p[1], N, N, b.p[2]],
    "ma_invert_flow": lambda b: [b.p[0], N, N, 5, 1e-3, b.p[1], None, None],
    "ma_transform_points": lambda b: [b.p[0], 4, b.p[1], N, N, None, None, 0, 0, 0, 5, 1e-4, b.p[2], b.p[3], b.p[4]],
    "ma_transform_points_grid": lambda b: [b.p[0], 4, b.p[1], N, N, 4, None, None, 0, 0, 0, 5, 1e-4, b.p[2], b.p[3], b.p[4]],
    "ma_flow_grid_sample": lambda b: [b.p[0], N, N, 4, b.p[1]],
    "ma_flow_grid_expand": lambda b: [b.p[0], N, N, 4, b.p[1]],
    "ma_flow_grid_error": lambda b: [b.p[0], b.p[1], N, N, 4, N, N, 0.1, b.f, b.ll, b.ll2],
    "ma_smooth_flow": lambda b: [b.p[0], N, N, b.taps, 1, None, 0, N, N, 0, 0.0, b.p[1], None],
    "ma_flow_fold_mask": lambda b: [b.p[0], N, N, 0, b.p[1], None],
    "ma_median_flow": lambda b: [b.p[0], N, N, 1, None, 0, N, N, 0, 0.5, 0, b.p[1], None, None],
    "ma_fill_flow": lambda b: [b.p[0], N, N, None, 0, N, N, b.p[1], None],
    "ma_flow_refine_step": lambda b: [b.p[0], 0, b.p[1], N, N, b.taps, 1, 1.0, None, 0, 1.0, b.p[2], b.p[3], None],
    "ma_flow_affine_moments": lambda b: [b.p[0], N, N, None, 0, N, N, None, 0.0, b.d, b.ll],
    "ma_flow_affine_apply": lambda b: [b.p[0], N, N, b.m6, b.p[1]],
    "ma_landmark_flow": lambda b: [b.p[0], 0, b.m6, 0.0, 0.0, 1.0, N, N, 1, b.p[1]],
    "ma_landmark_points": lambda b: [b.p[0], 0, b.m6, 0.0, 0.0, 1.0, b.p[1], 4, b.p[2]],
    "ma_pyr_up_flow": lambda b: [b.p[0], N // 2, N // 2, 1.0, b.p[1], N, N],
    "ma_qc_flow_grid": lambda b: [b.p[0], N, N, N, N, b.d, b.ll, b.ll2, b.d2, b.d3],
}


@pytest.fixture(scope="module")
def bufs(ctx):
    return Bufs(ctx)


@pytest.mark.parametrize("entry,param,nbytes,pos", REJECT, ids=[f"{e}:{p}" for e, p, _, _ in REJECT])
def test_a_pointer_below_the_rule_is_refused_before_any_launch(ctx, bufs, entry, param, nbytes, pos):
    from microaligner_amd import _lib as L
    fn = getattr(ctx.lib, entry)
    good = CALLS[entry](bufs)
    assert isinstance(good[pos - 1], int) and good[pos - 1] % 64 == 0, "the valid call passes an aligned device pointer there"
    bad = list(good)
    bad[pos - 1] = good[pos - 1] + nbytes // 2
    rc = fn(ctx.handle, *bad)
    msg = ctx.lib.ma_last_error().decode()
    assert rc == L.MA_EINVAL, (rc, msg)
    assert f"{param} must be {nbytes}-byte aligned" in msg, msg
    rc = fn(ctx.handle, *good)
    assert rc == L.MA_OK, (rc, ctx.lib.ma_last_error().decode())
    ctx.sync()


# ---- below the rule, where the check is the size of the element ----------------------------------------------------------------
# (source file, parameter, the size as the source writes it): every MA_REQUIRE_ALIGNED whose size is no literal.  The size
# follows an argument of the call, so REJECT's one row per parameter cannot hold it; BELOW lists the pointers instead.
ELEMENT_SIZED = [
    ("local_norm.hip", "img", "img_elem"),
    ("local_norm.hip", "weight", "weight_elem"),
    ("local_norm.hip", "out_f32", "sizeof(float)"),
]

# (parameter, dtype code of the image, weight kind, bytes of the element, what the pointer is moved by)
BELOW = [("img", 1, 0, 2, 1), ("img", 2, 0, 4, 1), ("img", 2, 0, 4, 2), ("weight", 0, 1, 4, 1), ("weight", 0, 1, 4, 2),
         ("out_f32", 0, 0, 4, 1), ("out_f32", 0, 0, 4, 2)]


def below_call(p, dtype, kind, taps, counts):
    """the arguments after ctx of a valid ma_normalize_local on an N x N image, by the names BELOW uses, in the order of the
    prototype; p: four device pointers (the image, the weight, the two outputs)"""
    return dict(img=p[0], dtype=dtype, H=N, W=N, taps=taps, r=1, floor=1.0, clip=4.0, weight=p[1] if kind else None,
                kind=kind, ms=0.0, out_f32=p[2], out_u8=p[3], counts=counts)


@pytest.mark.parametrize("param,dtype,kind,nbytes,by", BELOW, ids=[f"{p}:{n}-byte element + {b}" for p, _, _, n, b in BELOW])
def test_a_pointer_below_the_rule_is_refused_before_any_launch_element_sized(ctx, param, dtype, kind, nbytes, by):
    from microaligner_amd import _lib as L
    z = [ctx.zeros((16384,), F32) for _ in range(4)]
    sentinel = np.full(N * N, 7, F32)
    L.check(ctx.lib.ma_memcpy_h2d(ctx.handle, z[2].ptr, sentinel.ctypes.data, sentinel.nbytes))
    taps = (C.c_float * 2)(0.5, 0.25)
    counts = (C.c_longlong * 4)(-1, -1, -1, -1)
    good = below_call([a.ptr for a in z], dtype, kind, taps, counts)
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
    import _local_norm_ref as R
    from microaligner_amd import _lib as L
    from test_gpu_flow_smooth import taps_of
    SHAPE = G.SHAPE
    img = R.make_image(*SHAPE, np.uint8)
    mask = R.make_weight(*SHAPE)[1]
    taps, floor = taps_of(7), R.floor_of(np.uint8)
    exp = R.normalize_local_ref(img, taps, floor, 4.0, mask, 0.05)
    alloc = Shifted(ctx, "edge", None, type(ctx).empty)
    d_img, d_mask, out = (alloc.view(SHAPE, np.uint8, 1 if which == n else 16) for n in ("img", "mask", "out_u8"))
    for d, a in ((d_img, img), (d_mask, mask)):
        L.check(ctx.lib.ma_memcpy_h2d(ctx.handle, d.ptr, a.ctypes.data, a.nbytes))
    counts = (C.c_longlong * 4)()
    ctx._run(ctx.lib.ma_normalize_local, d_img.ptr, L.MA_U8, *SHAPE, taps.ctypes.data_as(C.POINTER(C.c_float)), 7, floor, 4.0,
             d_mask.ptr, L.MA_SMOOTH_WEIGHT_U8, 0.05, None, out.ptr, counts)
    assert (d_img.ptr if which == "img" else d_mask.ptr if which == "mask" else out.ptr) % 2 == 1
    G.assert_same((out.numpy(), tuple(counts)), (exp["u8"], exp["counts"]), which)
    assert not alloc.slack_damage()
