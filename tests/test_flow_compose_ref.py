"""The exact flow composition on the CPU (no GPU): the numpy float32 statement of include/microaligner_flowcompose.h
(tests/_flow_compose_ref.py) against identities, the oracle's cv2.remap, the float64 analytic composition and the border
rule; the accuracy of register() with the exact bookkeeping against the reference's, both stated over the oracle's
primitives; the FlowComposition key of the command-line config."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import oracle_threads  # noqa: E402
import _flow_compose_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import register_oracle as RO  # noqa: E402
from microaligner_amd import pipeline as P, synthetic  # noqa: E402

F32 = np.float32


def smooth_flow(H, W, amp=3.0, period=100.0, phase=0.0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    k = 2 * np.pi / period
    return np.stack([amp * np.sin(k * x + phase) * np.cos(k * y), amp * np.cos(k * x) * np.sin(k * y + phase)], -1).astype(F32)


def test_identities():
    rng = np.random.default_rng(0)
    t = rng.normal(0, 3, (37, 53, 2)).astype(F32)
    z = np.zeros_like(t)
    assert np.array_equal(R.compose_flows_ref(z, t), t)            # nothing so far: this level's flow
    assert np.array_equal(R.compose_flows_ref(t, z), t)            # a zero level flow: the flow so far, sampled on the grid
    assert np.array_equal(R.compose_flows_ref(t, -z), t)           # -0.0 + 0.0 is +0.0: equal as values
    first = np.empty_like(t)
    first[...] = (1.25, -2.5)
    second = np.empty_like(t)
    second[...] = (3.0, -7.0)                                       # integer valued: the samples fall on pixels
    out = R.compose_flows_ref(first, second)
    assert np.array_equal(out, np.broadcast_to(np.array([4.25, -9.5], F32), t.shape))


@pytest.mark.parametrize("shape", [(300, 420), (1, 1), (1, 77), (77, 1), (64, 257)])
def test_equals_second_plus_the_oracles_remap_of_the_clamped_map(shape):
    H, W = shape
    first, second = smooth_flow(H, W, 3.0, 100.0), smooth_flow(H, W, 4.0, 70.0, 1.0)
    cx, cy = R.clamped_map(second)
    exp = second + O.remap(first, np.ascontiguousarray(np.stack([cx, cy], -1)))
    assert np.array_equal(R.compose_flows_ref(first, second), exp)


def test_within_the_derived_bound_of_the_float64_analytic_composition():
    """first analytic and smooth, so first(p - second(p)) is known in float64.  Bound per component: the coordinate is
    quantised to 1/32 px, so off by at most 1/64 px per axis, times the first derivatives; the bilinear remainder is at
    most h^2 / 8 (h = 1 px) times the second derivatives per axis; 1e-5 for the float32 roundings."""
    H, W, amp, period = 300, 420, 3.0, 100.0
    k = 2 * np.pi / period
    second = smooth_flow(H, W, 2.5, 130.0, 0.7)
    first = smooth_flow(H, W, amp, period)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    sx, sy = x - second[..., 0].astype(np.float64), y - second[..., 1].astype(np.float64)
    inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
    exact = np.stack([amp * np.sin(k * sx) * np.cos(k * sy), amp * np.cos(k * sx) * np.sin(k * sy)], -1) + second
    err = np.abs(R.compose_flows_ref(first, second).astype(np.float64) - exact)[inside].max()
    # |f_x|_max + |f_y|_max = 2 amp k and |f_xx|_max + |f_yy|_max = 2 amp k^2 for both components
    bound = 2 * amp * k / 64 + 2 * amp * k * k / 8 + 1e-5
    print(f"analytic composition: max error {err:.4f} px, bound {bound:.4f} px")
    assert inside.mean() > 0.95 and err <= bound


def test_samples_that_leave_the_image_take_the_border_value():
    H, W = 40, 50
    rng = np.random.default_rng(1)
    first = rng.normal(0, 2, (H, W, 2)).astype(F32)
    for t, src in (((1000.0, 0.0), lambda y, x: (y, 0)), ((-1000.0, 0.0), lambda y, x: (y, W - 1)),
                   ((0.0, 1000.0), lambda y, x: (0, x)), ((0.0, -1000.0), lambda y, x: (H - 1, x)),
                   ((-1e9, -1e9), lambda y, x: (H - 1, W - 1))):
        second = np.empty_like(first)
        second[...] = t
        out = R.compose_flows_ref(first, second)
        for y, x in ((0, 0), (H - 1, W - 1), (17, 23)):
            assert np.array_equal(out[y, x], second[y, x] + first[src(y, x)])
    second = np.zeros_like(first)
    second[5, 6] = (np.nan, 1.0)
    second[7, 8] = (np.inf, -np.inf)
    out = R.compose_flows_ref(first, second)
    bad = ~np.isfinite(out).all(-1)
    assert bad.sum() == 2 and bad[5, 6] and bad[7, 8]             # a non-finite t: that pixel and no other
    assert np.isnan(out[5, 6, 0]) and out[5, 6, 1] == F32(1.0) + first[4, 0, 1]   # NaN x clamps to column 0
    assert out[7, 8, 0] == np.inf and out[7, 8, 1] == -np.inf


ACCURACY = dict(num_iterations=3, tile_size=1000, overlap=100)


@pytest.fixture(scope="module")
def pair_1024():
    return synthetic.make_pair(1024, 1024, seed=1)


@pytest.mark.parametrize("full_res", [True, False])
def test_exact_bookkeeping_is_more_accurate_than_the_references(pair_1024, full_res):
    """1024^2, num_pyr_lvl=3, window 99, no DOG, 64 px border left out: the median endpoint error of the exact flow is
    at most a quarter of the reference bookkeeping's (measured ratios 0.12 with the full-resolution level and 0.06
    without; the factor leaves 2x); without the full-resolution level the reference returns half the magnitude (Q2)."""
    ref, mov = pair_1024
    params = dict(ACCURACY, num_pyr_lvl=3, use_full_res_img=full_res, nthreads=oracle_threads())
    truth = np.stack(synthetic.displacement(1024, 1024, dtype=np.float64), -1)
    f_ref, rep_ref = RO.register(ref, mov, **params)
    f_ex, rep_ex = R.register_exact(ref, mov, **params)
    e_ref, e_ex = R.endpoint_error(f_ref, truth), R.endpoint_error(f_ex, truth)
    print(f"full_res={full_res}: reference median/p99/max {e_ref}, exact {e_ex}, accepted {[r[3] for r in rep_ref]} / "
          f"{[r[3] for r in rep_ex]}, zero flow {R.endpoint_error(np.zeros_like(f_ex), truth)}")
    assert f_ex.shape == (1024, 1024, 2) and f_ex.dtype == F32
    assert e_ex[0] <= 0.25 * e_ref[0]
    if not full_res:
        mag = lambda f: float(np.median(np.hypot(f[..., 0], f[..., 1])[64:-64, 64:-64]))
        ratio = mag(f_ex) / mag(f_ref)
        print(f"median |flow| exact / reference: {ratio:.3f}")
        assert 1.8 <= ratio <= 2.2


def _cfg(optflow_extra=None, feature_extra=None):
    reg = dict(NumberPyramidLevels=2, NumberIterationsPerLevel=3, TileSize=150, Overlap=30, NumberOfWorkers=0,
               UseFullResImage=True, UseDOG=False)
    cfg = {"Input": {"InputImagePaths": {"Cycle 1": "a.npy", "Cycle 2": "b.npy"}, "ReferenceCycle": 1, "ReferenceChannel": "0"},
           "Output": {"OutputDir": "out", "OutputPrefix": "exp_", "SaveOutputToCycleStack": True},
           "RegistrationParameters": {"OptFlowReg": dict(reg, **(optflow_extra or {}))}}
    if feature_extra is not None:
        cfg["RegistrationParameters"]["FeatureReg"] = dict(reg, **feature_extra)
    return cfg


def test_pipeline_config_takes_flow_composition_under_optflow_reg_only():
    base = P.PipelineConfig(_cfg()).optflow.optflow_kwargs()
    assert "flow_composition" not in base                                   # absent: the registrator's default, "reference"
    for v in ("reference", "exact"):
        kw = P.PipelineConfig(_cfg(dict(FlowComposition=v))).optflow.optflow_kwargs()
        assert kw == dict(base, flow_composition=v)
    with pytest.raises(ValueError, match="Field FlowComposition value"):
        P.PipelineConfig(_cfg(dict(FlowComposition="Exact")))
    for bad in (1, True, None, ["exact"]):
        with pytest.raises(TypeError, match="Field FlowComposition has wrong data type"):
            P.PipelineConfig(_cfg(dict(FlowComposition=bad)))
    with pytest.raises(ValueError, match="FlowComposition"):
        P.PipelineConfig(_cfg(feature_extra=dict(FlowComposition="exact")))
    assert "flow_composition" not in P.PipelineConfig(_cfg(feature_extra={})).feature.feature_kwargs()
