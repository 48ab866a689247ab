"""-m gpu: the exact flow composition on the device.  ma_compose_flows against the numpy float32 statement of
include/microaligner_flowcompose.h (tests/_flow_compose_ref.py) bit for bit; register() with
flow_composition = "exact" against the same level loop over the oracle's primitives; the default left as it is; the
plumbing of the new header."""
import importlib.util
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import oracle_threads  # noqa: E402
import _flow_compose_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import register_oracle as RO  # noqa: E402
from microaligner_amd import OptFlowRegistrator, _lib, compose_flows, synthetic  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_flowcompose.h")


def same_bits(got, exp):
    """equal as bit patterns, any NaN payload standing for NaN"""
    assert got.dtype == exp.dtype == F32 and got.shape == exp.shape
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(got.view(np.uint32)[~gn], exp.view(np.uint32)[~en])


def flows(H, W, kind, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    first = np.stack([3 * np.sin(x / 17.0) + 2 * np.cos(y / 23.0), 2.5 * np.cos(x / 13.0 + y / 31.0)], -1)
    first = (first + rng.normal(0, 0.3, first.shape)).astype(F32)
    if kind == "few_px":
        second = np.stack([2.7 + 1.5 * np.sin(x / 30.0) * np.cos(y / 50.0), -1.9 + 1.5 * np.cos(x / 40.0)], -1)
        second = (second + rng.normal(0, 0.2, second.shape)).astype(F32)
    elif kind == "hundreds_px":       # every sample leaves a small image: the clamps
        second = (rng.uniform(-900, 900, (H, W, 2))).astype(F32)
    else:                             # integer valued: the samples fall on pixels
        second = rng.integers(-6, 7, (H, W, 2)).astype(F32)
    return first, second


SHAPES = [(1, 1), (1, 300), (300, 1), (40, 255), (40, 256), (40, 257), (13, 64), (9, 700), (7, 5), (2049, 1031)]


@pytest.mark.parametrize("kind", ["few_px", "hundreds_px", "integers"])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_numpy_statement_bit_for_bit(ctx, shape, kind):
    first, second = flows(*shape, kind, seed=shape[0] + shape[1])
    got = ctx.compose_flows(ctx.asdevice(first), ctx.asdevice(second)).numpy()
    assert same_bits(got, R.compose_flows_ref(first, second))


def test_identities_on_the_device(ctx):
    first, second = flows(123, 211, "few_px")
    z = np.zeros_like(first)
    assert np.array_equal(compose_flows(z, second), second)
    assert np.array_equal(compose_flows(first, z), first)


def test_non_finite_values_stay_where_they_are(ctx):
    H, W = 67, 301
    first, second = flows(H, W, "few_px", 5)
    second[5, 6] = (np.nan, 1.0)
    second[7, 8] = (np.inf, -np.inf)
    second[66, 300] = (-np.inf, np.nan)
    second[20, 20] = (1e30, -1e30)
    exp0 = R.compose_flows_ref(first, second)
    got = ctx.compose_flows(ctx.asdevice(first), ctx.asdevice(second)).numpy()
    assert same_bits(got, exp0)
    bad = ~np.isfinite(got).all(-1)
    assert bad.sum() == 3 and bad[5, 6] and bad[7, 8] and bad[66, 300]      # a non-finite t: that pixel and no other
    first[30, 40] = (np.nan, 0.0)
    first[0, 0] = (np.inf, -np.inf)
    first[50, 100] = (-np.inf, 3.0)
    exp = R.compose_flows_ref(first, second)
    got = ctx.compose_flows(ctx.asdevice(first), ctx.asdevice(second)).numpy()
    assert same_bits(got, exp)
    # only the outputs whose four taps include a non-finite value of first changed
    cx, cy = R.clamped_map(second)
    qx, qy = np.rint(cx * F32(32)).astype(np.int64) >> 5, np.rint(cy * F32(32)).astype(np.int64) >> 5
    touched = np.zeros((H, W), bool)
    for py, px in ((30, 40), (0, 0), (50, 100)):
        touched |= ((qx == px) | (np.minimum(qx + 1, W - 1) == px)) & ((qy == py) | (np.minimum(qy + 1, H - 1) == py))
    changed = ~(np.isfinite(got).all(-1)) & ~bad
    assert changed.any() and not (changed & ~touched).any()
    assert same_bits(got[~touched], exp0[~touched])


def test_out_may_be_second_and_bad_arguments_are_refused(ctx):
    first, second = flows(203, 517, "few_px", 9)
    exp = R.compose_flows_ref(first, second)
    d1, d2 = ctx.asdevice(first.copy()), ctx.asdevice(second.copy())
    H, W = first.shape[:2]
    call = lambda *a: ctx._run(ctx.lib.ma_compose_flows, *a)
    call(d1.ptr, d2.ptr, H, W, d2.ptr)                      # in place over second
    assert same_bits(d2.numpy(), exp)
    d2 = ctx.asdevice(second.copy())
    for args in ((None, d2.ptr, H, W, d2.ptr), (d1.ptr, None, H, W, d2.ptr), (d1.ptr, d2.ptr, H, W, None),
                 (d1.ptr, d2.ptr, 0, W, d2.ptr), (d1.ptr, d2.ptr, H, 0, d2.ptr), (d1.ptr, d2.ptr, -1, W, d2.ptr),
                 (d1.ptr, d2.ptr, (1 << 24) + 1, 1, d2.ptr), (d1.ptr, d2.ptr, 1, (1 << 24) + 1, d2.ptr),
                 (d1.ptr, d2.ptr, H, W, d1.ptr)):            # out == first
        with pytest.raises(ValueError):
            call(*args)
    assert ctx.lib.ma_compose_flows(None, d1.ptr, d2.ptr, H, W, d2.ptr) == _lib.MA_EINVAL
    assert same_bits(d1.numpy(), first) and same_bits(d2.numpy(), second)     # a refused call wrote nothing


def test_entry_points_take_numpy_and_device_arrays(ctx):
    first, second = flows(150, 333, "few_px", 3)
    exp = R.compose_flows_ref(first, second)
    out = compose_flows(first, second)
    assert isinstance(out, np.ndarray) and same_bits(out, exp)
    dout = compose_flows(ctx.asdevice(first), ctx.asdevice(second))
    assert isinstance(dout, DeviceArray) and dout.shape == first.shape and same_bits(dout.numpy(), exp)
    for a, b in ((first.astype(np.float64), second), (first, second.astype(np.float64)), (first[..., 0], second[..., 0]),
                 (first[:-1], second), (np.zeros((4, 4, 3), F32), np.zeros((4, 4, 3), F32))):
        with pytest.raises(ValueError):
            compose_flows(np.ascontiguousarray(a), np.ascontiguousarray(b))
    with pytest.raises(ValueError):
        ctx.compose_flows(ctx.asdevice(first), ctx.asdevice(np.ascontiguousarray(second[:, :-1])))


# ---- register() -----------------------------------------------------------------------------------------------------
def _golden_cases():
    spec = importlib.util.spec_from_file_location("_make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CASES


CASES = dict(_golden_cases())
ACCURACY = dict(num_pyr_lvl=3, num_iterations=3, tile_size=1000, overlap=100)
CASES["accuracy_1024_fullres"] = dict(shape=(1024, 1024), dtype="float32", seed=1, params=dict(ACCURACY, use_full_res_img=True))
CASES["accuracy_1024_nofull"] = dict(shape=(1024, 1024), dtype="float32", seed=1, params=dict(ACCURACY, use_full_res_img=False))
_CPU = {}


def inputs(case):
    make = synthetic.make_unrelated_pair if case.get("unrelated") else synthetic.make_pair
    return make(*case["shape"], case["seed"], case["dtype"])


def cpu_exact(name, fused=False):
    if (name, fused) not in _CPU:
        ref, mov = inputs(CASES[name])
        _CPU[name, fused] = R.register_exact(ref, mov, fused=fused, dog_flags=O.DOG_FUSED if fused else 0,
                                             nthreads=oracle_threads(), **CASES[name]["params"])
    return _CPU[name, fused]


def make_reg(params):
    reg = OptFlowRegistrator()
    reg.verbose = False
    for k, v in params.items():
        setattr(reg, k, v)
    return reg


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_register_exact_equals_the_cpu_statement(name, fused):
    """flows bit-identical, decisions equal, MI scores within the 1e-12 that the gate's doubles keep against the oracle's
    everywhere in this suite; fused: Farneback's window blur and the dog() chain in the fused multiply-add model."""
    exp, reports = cpu_exact(name, fused)
    ref, mov = inputs(CASES[name])
    reg = make_reg(dict(CASES[name]["params"], flow_composition="exact", muladd_fused=fused, dog_muladd_fused=fused))
    reg.ref_img, reg.mov_img = ref, mov
    got = reg.register()
    assert [r.factor for r in reg.level_reports] == [r[0] for r in reports]
    assert [r.accepted for r in reg.level_reports] == [r[3] for r in reports]
    np.testing.assert_allclose([(r.mi_after, r.mi_before) for r in reg.level_reports], [r[1:3] for r in reports],
                               rtol=0, atol=1e-12)
    assert isinstance(got, np.ndarray) and got.shape == tuple(CASES[name]["shape"]) + (2,)
    assert same_bits(got, exp)


def test_the_case_list_covers_every_branch_of_the_bookkeeping():
    """from the CPU statement's own reports, so that the list cannot quietly stop covering a branch"""
    seen = set()
    for name, case in CASES.items():
        p = dict(tile_size=1000, overlap=100, use_full_res_img=False, num_pyr_lvl=4)
        p.update(case["params"])
        acc = [r[3] for r in cpu_exact(name)[1]]
        n = len(acc)
        if not acc[0]:
            seen.add("first level rejected")
        if n >= 3 and not all(acc[1:-1]):
            seen.add("middle level rejected")
        if n >= 2 and not acc[-1]:
            seen.add("last level rejected")
        if n >= 2 and acc[0] and acc[1]:
            seen.add("composition")
        if n == 1:
            seen.add("single level")
        ref = inputs(case)[0]
        levels, _ = RO.image_pyramid(ref, p["num_pyr_lvl"], p["use_full_res_img"])
        if any(max(lv.shape) / p["tile_size"] >= 2 for lv in levels):
            seen.add("tiled level")
        if case["dtype"] == "uint8":
            seen.add("uint8 pair")
        if not p["use_full_res_img"]:
            seen.add("no full-resolution level")
    assert seen == {"first level rejected", "middle level rejected", "last level rejected", "composition", "single level",
                    "tiled level", "uint8 pair", "no full-resolution level"}


def test_exact_is_more_accurate_on_the_tiled_2048_pair():
    """2048^2, num_pyr_lvl=3, full-resolution level, tile 1000 / overlap 100 (tiled levels): median endpoint error of the
    exact flow at most a quarter of the reference bookkeeping's (0.043 against 0.820 px on the CPU statement)."""
    ref, mov = synthetic.make_pair(2048, 2048, seed=1)
    truth = np.stack(synthetic.displacement(2048, 2048, dtype=np.float64), -1)
    params = dict(ACCURACY, use_full_res_img=True)
    err = {}
    for mode in ("reference", "exact"):
        reg = make_reg(dict(params, flow_composition=mode))
        reg.ref_img, reg.mov_img = ref, mov
        err[mode] = R.endpoint_error(reg.register(), truth)
        print(mode, "median / p99 / max px:", err[mode], [r.accepted for r in reg.level_reports])
    assert err["exact"][0] <= 0.25 * err["reference"][0]


@pytest.mark.parametrize("name", ["fullres_dog_t100", "reject_mid_s38"])
def test_reference_composition_is_the_default_bit_for_bit(name):
    ref, mov = inputs(CASES[name])
    out = {}
    for engine in ("c", "python"):
        for mode in (None, "reference"):
            reg = make_reg(dict(CASES[name]["params"], engine=engine))
            assert reg.flow_composition == "reference"
            if mode:
                reg.flow_composition = mode
            reg.ref_img, reg.mov_img = ref, mov
            out[engine, mode] = (reg.register(), [(r.factor, r.mi_after, r.mi_before, r.accepted) for r in reg.level_reports])
    exp, reports = RO.register(ref, mov, **CASES[name]["params"])
    for flow, rep in out.values():
        assert same_bits(flow, exp) and rep == out["c", None][1] and [r[3] for r in rep] == [r[3] for r in reports]
    assert not np.array_equal(exp, cpu_exact(name)[0])       # and the exact flow is another flow


def test_unknown_flow_composition_is_refused_before_any_device_work(monkeypatch):
    from microaligner_amd.optflow_reg import optflow_registrator as M

    def no_device(*a, **k):
        raise AssertionError("validation must not reach the device")
    monkeypatch.setattr(M, "get_context", no_device)
    ref, mov = synthetic.make_pair(200, 220, seed=2)
    for bad in ("Exact", "", None, 1):
        reg = make_reg(dict(flow_composition=bad))
        reg.ref_img, reg.mov_img = ref, mov
        with pytest.raises(ValueError, match="flow_composition"):
            reg.register()


def test_register_pairs_passes_flow_composition_through():
    from microaligner_amd import parallel
    params = dict(num_pyr_lvl=2, use_full_res_img=True, tile_size=100, overlap=20, flow_composition="exact")
    pairs = [synthetic.make_pair(420, 404, seed) for seed in (2, 3)]
    flows_ = parallel.register_pairs(pairs, params)
    for (ref, mov), f in zip(pairs, flows_):
        reg = make_reg(params)
        reg.ref_img, reg.mov_img = ref, mov
        single = reg.register()
        assert same_bits(np.asarray(f), single)
        reg = make_reg(dict(params, flow_composition="reference"))
        reg.ref_img, reg.mov_img = ref, mov
        assert not np.array_equal(reg.register(), single)


# ---- plumbing -------------------------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))


def test_header_library_and_bindings_agree():
    lib = _lib.load()
    names = _declared(HEADER)
    assert names == ["ma_compose_flows"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_flowcompose.h but not exported"
    assert sorted(_lib.FLOWCOMPOSE_SIGNATURES) == names
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES]
    assert not any(set(_lib.FLOWCOMPOSE_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_hip.h"' in open(HEADER).read()


def test_flow_compose_stays_out_of_the_measured_path_hash(tmp_path, monkeypatch):
    from microaligner_amd import build
    assert "flow_compose.hip" in build.SOURCES and HEADER not in [os.path.abspath(h) for h in build.HEADERS]
    assert os.path.abspath(build.SOURCE_HEADERS["flow_compose.hip"][0]) == HEADER
    before = build.source_hash()
    assert _lib.source_hash() == before                      # the loaded library is this tree's
    csrc = tmp_path / "csrc"
    shutil.copytree(build.CSRC, csrc)
    headers = [str((csrc if os.path.samefile(os.path.dirname(h), build.CSRC) else tmp_path) / os.path.basename(h))
               for h in build.HEADERS]
    shutil.copy(os.path.join(ROOT, "include", "microaligner_hip.h"), tmp_path / "microaligner_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "HEADERS", headers)
    assert build.source_hash() == before
    with open(csrc / "flow_compose.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() == before
    with open(csrc / "remap.hip", "a") as f:
        f.write("\n// edited\n")
    assert build.source_hash() != before
