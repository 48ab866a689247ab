"""-m gpu: the alignment moments on the device against the numpy statement of include/microaligner_direct.h
(tests/_direct_affine_ref.py) -- counts exactly, sums within the bound every order of summation keeps, two calls the same
bits -- and align_affine end to end against the same loop over the statement's moments."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _direct_affine_ref as R  # noqa: E402
import test_direct_affine_ref as T  # noqa: E402
from microaligner_amd import DirectAffineInfo, Warper, _lib, align_affine  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64, U8, U16 = np.float32, np.float64, np.uint8, np.uint16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_direct.h")

# 37 x 515: three tile columns of 256, the last ragged, less than one tile row; 96 x 161: two tile rows of 64, an odd width;
# the degenerate ones: 1 x 1 has no inside pixel, 2 x 2 has one only where the sample falls on pixel (0, 0) exactly
SHAPES = [(37, 515), (96, 161), (1, 1), (2, 2)]
DTYPES = (U8, U16, F32)
U = 2.0 ** -53
# device against the numpy loop: they differ only by the order of summation (measured on MI355X: 1.6e-14 px at most)
E2E_TOL = 1e-6


def images(shape, ref_dtype, mov_dtype, seed=5):
    """a pair under a small similarity, whatever the shape"""
    M = R.true_matrix(shape, 1.0, 1.005, (1.5, -0.75))
    ref, mov = R.make_pair(shape, M, seed, ref_dtype=ref_dtype, mov_dtype=mov_dtype)
    return ref, mov, M


def make_weight(kind, shape, seed=7):
    rng = np.random.default_rng(seed)
    H, W = shape
    if kind == "none":
        return None
    if kind == "u8":
        return (rng.random(shape) < 0.7).astype(U8) * rng.integers(1, 256, shape).astype(U8)
    w = rng.uniform(0.25, 2.0, shape).astype(F32)
    w[rng.random(shape) < 0.3] = 0
    for k, v in enumerate((np.nan, -1.0, 0.0, np.inf, -np.inf, -0.0, 1e-40)):
        w[(3 + 7 * k) % H, (2 + 29 * k) % W] = v
    return w


def check_moments(ctx, ref, mov, M, gain=1.0, bias=0.0, weight=None, clip=None):
    """counts equal and adding up to H * W; every sum within (n + 1) 2^-53 sum |term| of the fsum; a second call gives the
    same bits"""
    exp, exp_counts, exp_abs = R.moments_ref(ref, mov, M, gain, bias, weight, clip)
    d_ref, d_mov = ctx.asdevice(ref), ctx.asdevice(mov)
    d_w = None if weight is None else ctx.asdevice(weight)
    sums, counts = ctx.direct_affine_moments(d_ref, d_mov, M, gain, bias, d_w, clip)
    assert sums.shape == (31,) and sums.dtype == F64 and counts.shape == (5,) and counts.dtype == np.int64
    assert np.array_equal(counts, exp_counts), (counts, exp_counts)
    assert counts.sum() == ref.shape[0] * ref.shape[1]
    bound = (exp_counts[0] + 1) * U * exp_abs
    err = np.abs(sums - exp)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    if exp_counts[0] == 0:
        assert not sums.any()
    again = ctx.direct_affine_moments(d_ref, d_mov, M, gain, bias, d_w, clip)
    assert np.array_equal(again[0].view(np.uint64), sums.view(np.uint64)) and np.array_equal(again[1], counts)
    return sums, counts


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_equal_the_statement(ctx, shape):
    """every pair of dtypes x every weight kind, with a gain and a bias"""
    used = 0
    for rd in DTYPES:
        for md in DTYPES:
            ref, mov, M = images(shape, rd, md)
            for kind in ("none", "f32", "u8"):
                _, counts = check_moments(ctx, ref, mov, M, 0.9, 2.0, make_weight(kind, shape))
                used += counts[0]
    assert (used > 0) == (shape[0] > 2)
    if shape == (2, 2):
        ref, mov, _ = images(shape, F32, U16)
        _, counts = check_moments(ctx, ref, mov, np.eye(2, 3))
        assert counts.tolist() == [1, 3, 0, 0, 0]


def test_moments_with_clipping(ctx):
    """a clip at the median residual trims about half; clips that take everything and nothing; clip <= 0 through the C
    entry is no clipping"""
    ref, mov, M = images((96, 161), U16, F32)
    Mk = 0.5 * np.eye(2, 3) + 0.5 * M
    f = R.pixel_fields(ref, mov, Mk, 1.1, -3.0)
    half = float(np.median(np.abs(f["e"][f["cls"] == R.USED])))
    w = make_weight("f32", ref.shape)
    seen = []
    for clip in (half, 1e-9, 1e30, float("inf")):
        for weight in (None, w):
            _, counts = check_moments(ctx, ref, mov, Mk, 1.1, -3.0, weight, clip)
            seen.append((clip, int(counts[0]), int(counts[4])))
    assert 0.4 < seen[0][2] / (seen[0][1] + seen[0][2]) < 0.6
    assert seen[2][1] == 0 and seen[2][2] > 0 and seen[4][2] == 0 and seen[6][2] == 0
    none = check_moments(ctx, ref, mov, Mk, 1.1, -3.0)
    d_ref, d_mov = ctx.asdevice(ref), ctx.asdevice(mov)
    sums, counts = (C.c_double * 31)(), (C.c_longlong * 5)()
    m6 = (C.c_double * 6)(*Mk.ravel())
    for clip in (0.0, -2.0, float("nan")):
        ctx._run(ctx.lib.ma_direct_affine_moments, d_ref.ptr, 1, d_mov.ptr, 2, 96, 161, m6, 1.1, -3.0, None, 0, clip, sums, counts)
        assert list(counts) == none[1].tolist() and np.array_equal(np.array(sums[:]).view(np.uint64), none[0].view(np.uint64))


def test_moments_with_pixels_and_weights_that_are_not_finite(ctx):
    """NaN / Inf pixels of a float32 image in either role (a bad moving pixel spoils up to four samples), with a weight
    that holds NaN, 0, negative and infinite entries"""
    shape = (96, 161)
    vals = (np.nan, np.inf, -np.inf, np.nan, np.inf, 3e38)
    for role in ("ref", "mov", "both"):
        ref, mov, M = images(shape, F32, F32)
        for k, v in enumerate(vals):
            if role in ("ref", "both"):
                ref[(5 + 11 * k) % 96, (6 + 37 * k) % 161] = v
            if role in ("mov", "both"):
                mov[(9 + 13 * k) % 96, (4 + 31 * k) % 161] = v
        for kind in ("none", "f32"):
            _, counts = check_moments(ctx, ref, mov, M, 1.0, 0.0, make_weight(kind, shape))
            assert counts[2] >= {"ref": 4, "mov": 12, "both": 16}[role]
    ref, mov, M = images(shape, U8, F32)
    mov[40:44] = np.nan
    assert check_moments(ctx, ref, mov, M)[1][2] > 4 * 150


def test_moments_with_samples_outside(ctx):
    """a 7 degree rotation and a shift that puts about a third of the samples outside, matrices that put all of them
    outside, and samples at 2^40 and beyond the integers"""
    for shape, shift in (((96, 161), (45.0, 0.0)), ((37, 515), (20.0, 0.0))):
        ref, mov, _ = images(shape, U8, U16)
        M7 = R.true_matrix(shape, 7.0, 1.0, shift)
        _, counts = check_moments(ctx, ref, mov, M7, weight=make_weight("u8", shape))
        share = counts[1] / (shape[0] * shape[1])
        assert 0.25 < share < 0.5, share
        for away in (np.array([[1.0, 0, 2.0 * shape[1]], [0, 1.0, 0]]), np.array([[1.0, 0, 0], [0, 1.0, -1.0 - shape[0]]]),
                     np.array([[1.0, 0, 2.0 ** 40], [0, 1.0, 0]]), np.array([[1e300, 0, 1e300], [0, 1e300, 0]]),
                     np.array([[0.0, 0, -0.5], [0, 0.0, 3.0]])):
            _, counts = check_moments(ctx, ref, mov, away)
            assert counts.tolist() == [0, shape[0] * shape[1], 0, 0, 0]


E2E_CASES = ["similarity 96x161", "similarity uint8", "affine 37x515", "affine uint8", "affine 200x232, two levels",
             "affine uint8 200x232, two levels, uint8 mask"]


def check_against_the_loop(got, info, exp_info, M, shape, recorded):
    """the device's result against the numpy loop's and against the truth"""
    assert isinstance(info, DirectAffineInfo) and got.shape == (2, 3) and got.dtype == F64
    dev = R.corner_error(info.matrix, exp_info.matrix, shape)
    err = R.corner_error(info.matrix, M, shape)
    print(f"corner positions against the numpy loop {dev:.3g} px, against the truth {err:.5f} px")
    assert dev <= E2E_TOL
    assert [(lv.passes, lv.rejected) for lv in info.levels] == [(lv.passes, lv.rejected) for lv in exp_info.levels]
    assert [lv.counts for lv in info.levels] == [lv.counts for lv in exp_info.levels]
    assert info.accepted and info.converged and err <= T.allowance(recorded)
    assert np.abs(got - R.inverse(info.matrix)).max() <= 1e-12


@pytest.mark.parametrize("name", E2E_CASES)
def test_align_affine_follows_the_numpy_loop(ctx, name):
    """numpy in and DeviceArray in give the same matrix; the last case takes uint8 images and a uint8 mask through two
    levels (the mask is a float32 map below full size, made on the device)"""
    ref, mov, M, model, recorded = T.pair(name)
    _, exp_info = T.statement_result(name)
    weight = T.case_weight(name)
    got, info = align_affine(ref, mov, model, weight=weight, return_info=True)
    check_against_the_loop(got, info, exp_info, M, ref.shape, recorded)
    plain = align_affine(ctx.asdevice(ref), ctx.asdevice(mov), model, weight=None if weight is None else ctx.asdevice(weight))
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, got)


def test_align_affine_from_a_start_with_a_weight_and_a_clip(ctx):
    """tmat= from a perturbed truth, a float32 weight, a clip: the same loop as the statement's"""
    for (ref, mov, M, start, kw), (_, exp_info) in zip(T.start_scenarios(), T.start_results()):
        got, info = align_affine(ctx.asdevice(ref), mov, "affine", tmat=start, return_info=True,
                                 **dict(kw, **({"weight": ctx.asdevice(kw["weight"])} if kw else {})))
        check_against_the_loop(got, info, exp_info, M, ref.shape, T.START_RECORDED)
        assert R.corner_error(R.inverse(start), M, ref.shape) > 1.0
    assert info.gain == 1.0 and info.bias == 0.0 and info.levels[0].counts[4] >= 250


def test_align_affine_on_dog_labels(ctx):
    """labels="dog" is align_affine on the device's own labels, and recovers the matrix within the statement's allowance"""
    ref, mov, mask, M = T.dog_pair()
    got, info = align_affine(ref, mov, "similarity", weight=mask, labels="dog", return_info=True)
    a, b = ctx.dog_u8(ctx.asdevice(ref)), ctx.dog_u8(ctx.asdevice(mov))
    same, same_info = align_affine(a, b, "similarity", weight=mask, return_info=True)
    assert np.array_equal(got, same) and info.levels == same_info.levels
    err = R.corner_error(info.matrix, M, ref.shape)
    print(f"dog labels: corner error {err:.5f} px, gain {info.gain:.4f}, bias {info.bias:.3f}")
    assert info.accepted and info.converged and err <= T.allowance(T.DOG_RECORDED)
    exp_info = R.align_ref(a.numpy(), b.numpy(), "similarity", weight=mask)[1]
    assert R.corner_error(info.matrix, exp_info.matrix, ref.shape) <= E2E_TOL


def test_nothing_inside_is_not_accepted(ctx):
    ref, mov, M, _, _ = T.pair("similarity uint8")
    start = R.inverse(np.array([[1.0, 0.0, 2.0 * ref.shape[1]], [0.0, 1.0, 0.0]]))
    got, info = align_affine(ref, mov, "affine", tmat=start, return_info=True)
    assert info.accepted is False and info.levels[-1].empty and info.used_share == 0.0 and np.array_equal(got, start)
    got, info = align_affine(ref, mov, "affine", weight=np.zeros(ref.shape, F32), return_info=True)
    assert info.accepted is False and np.array_equal(got, np.eye(2, 3))


def test_the_result_serves_the_warper(ctx):
    """Warper(tmat=result) with linear interpolation and a zero flow brings the moving image closer to the reference than
    the starting matrix does (RMS over the pixels 8 px inside the border)"""
    ref, mov, M, model, _ = T.pair("similarity 96x161")
    start = R.inverse(M + np.array([[0.002, -0.001, 0.8], [0.001, 0.003, -0.6]]))
    result = align_affine(ref, mov, model, tmat=start)

    def rms(tmat):
        w = Warper()
        w.image, w.flow, w.tmat, w.interpolation = mov, np.zeros(ref.shape + (2,), F32), tmat, "linear"
        out = w.warp()
        return float(np.sqrt(np.mean((out.astype(F64) - ref)[8:-8, 8:-8] ** 2)))
    before, after = rms(start), rms(result)
    print(f"RMS difference to the reference: {before:.4f} with the start, {after:.4f} with the result")
    assert after < before


def test_the_pipelines_direct_refine_logs_and_returns_the_refined_matrix(ctx):
    from microaligner_amd import pipeline
    ref, mov, M, start, _ = T.start_scenarios()[0]
    lines = []
    out = pipeline.refine_feature_matrix(ref, mov, start, "affine", lines.append)
    assert np.array_equal(out, align_affine(ref, mov, "affine", tmat=start))
    assert len(lines) == 1 and "accepted True" in lines[0] and "affine" in lines[0]
    moved = float(re.search(r"up to ([0-9.]+) px", lines[0]).group(1))
    assert abs(moved - R.corner_error(out, start, ref.shape)) <= 1e-3 and moved > 1.0
    away = R.inverse(np.array([[1.0, 0.0, 2.0 * ref.shape[1]], [0.0, 1.0, 0.0]]))
    assert np.array_equal(pipeline.refine_feature_matrix(ref, mov, away, "similarity", lines.append), away)
    assert "accepted False" in lines[1] and "moved by up to 0.000 px" in lines[1]


def test_a_mask_becomes_the_float32_map_of_its_weights(ctx):
    """odd sizes, so that the last thread's four pixels are ragged; one pixel; more than one block"""
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (3, 5), (37, 515), (200, 232)):
        mask = (rng.random(shape) < 0.6).astype(U8) * rng.integers(1, 256, shape).astype(U8)
        out = ctx.mask_weight(ctx.asdevice(mask))
        assert out.shape == shape and out.dtype == F32 and np.array_equal(out.numpy(), (mask != 0).astype(F32))
    d, o = ctx.asdevice(np.ones((4, 4), U8)), ctx.empty((4, 4), F32)
    for args in ((None, 16, o.ptr), (d.ptr, 16, None), (d.ptr, 0, o.ptr), (d.ptr, 1 << 42, o.ptr)):
        with pytest.raises(ValueError):
            ctx._run(ctx.lib.ma_direct_mask_weight, *args)
    for bad in (np.ones((4, 4), U8), ctx.asdevice(np.ones((4, 4), F32))):
        with pytest.raises(ValueError):
            ctx.mask_weight(bad)


def test_bad_arguments_are_refused_by_the_c_entry(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    ref, mov, M = images((H, W), F32, U8)
    d_ref, d_mov, d_w = ctx.asdevice(ref), ctx.asdevice(mov), ctx.asdevice(np.ones((H, W), F32))
    sums, counts = (C.c_double * 31)(), (C.c_longlong * 5)()
    m6 = lambda *v: (C.c_double * 6)(*v)                                                       # noqa: E731
    ok = dict(ref=d_ref.ptr, rdt=2, mov=d_mov.ptr, mdt=0, H=H, W=W, M=m6(1, 0, 0, 0, 1, 0), gain=1.0, bias=0.0, weight=None,
              kind=0, clip=0.0, sums=sums, counts=counts)
    mo = lambda **kw: ctx._run(ctx.lib.ma_direct_affine_moments, *dict(ok, **kw).values())     # noqa: E731
    mo()
    assert sum(counts) == H * W and counts[0] == (H - 1) * (W - 1)
    mo(weight=d_w.ptr, kind=1, clip=2.0)
    for kw in (dict(ref=None), dict(mov=None), dict(M=None), dict(sums=None), dict(counts=None), dict(H=0), dict(W=0),
               dict(H=-1), dict(H=big), dict(W=big), dict(rdt=-1), dict(rdt=3), dict(mdt=3), dict(kind=-1), dict(kind=3),
               dict(kind=4), dict(kind=1), dict(kind=2), dict(M=m6(1, 0, float("nan"), 0, 1, 0)),
               dict(M=m6(1, 0, 0, 0, float("inf"), 0)), dict(gain=float("nan")), dict(gain=float("inf")),
               dict(bias=float("-inf"))):
        with pytest.raises(ValueError):
            mo(**kw)
    assert ctx.lib.ma_direct_affine_moments(None, *ok.values()) == _lib.MA_EINVAL


def test_entry_points_refuse_before_any_device_call(ctx, monkeypatch):
    ref, mov, M = images((20, 30), F32, F32)
    d_ref, d_mov = ctx.asdevice(ref), ctx.asdevice(mov)
    w31 = ctx.asdevice(np.ones((20, 31), F32))
    cells = ctx.asdevice(np.ones((3, 4), F32))
    calls = []
    monkeypatch.setattr(type(ctx), "_run", lambda self, fn, *a: calls.append(fn))
    monkeypatch.setattr(type(ctx), "empty", lambda self, *a: calls.append("empty"))
    for kw in (dict(mov=w31), dict(weight=w31), dict(weight=cells), dict(M=np.eye(3)), dict(M=np.full((2, 3), np.nan)),
               dict(gain=float("inf")), dict(clip=0.0)):
        with pytest.raises(ValueError):
            ctx.direct_affine_moments(**dict(dict(ref=d_ref, mov=d_mov, M=np.eye(2, 3)), **kw))
    for kw in (dict(mov_img=w31), dict(model="homography"), dict(weight=cells), dict(tmat=np.full((2, 3), np.inf)),
               dict(labels="u8"), dict(use_full_res_img=False), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            align_affine(**dict(dict(ref_img=d_ref, mov_img=d_mov), **kw))
    assert calls == []


def test_header_library_and_bindings_agree():
    import microaligner_amd
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_direct_affine_moments", "ma_direct_mask_weight"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in microaligner_direct.h but not exported"
        proto = re.search(r"\b" + n + r"\s*\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.DIRECT_SIGNATURES[n][1]), n
    assert sorted(_lib.DIRECT_SIGNATURES) == names
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES, _lib.FLOWCOMPOSE_SIGNATURES,
              _lib.FLOWINVERT_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.FLOWGRID_SIGNATURES, _lib.FLOWSMOOTH_SIGNATURES,
              _lib.FLOWAFFINE_SIGNATURES, _lib.TEXTURE_SIGNATURES]
    assert not any(set(_lib.DIRECT_SIGNATURES) & set(t) for t in others)
    for name, value in re.findall(r"\b(MA_[A-Z0-9_]+)\s+(\d+)\b", text):
        assert getattr(_lib, name) == int(value), name
    assert {"align_affine", "DirectAffineInfo"} <= set(microaligner_amd.__all__)
