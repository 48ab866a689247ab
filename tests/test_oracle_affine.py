"""transform_img_with_tmat: the numpy oracle (oracle/affine_oracle.py) against fixtures produced by the REAL
scikit-image 0.18.3 (tests/golden/make_affine_golden.py), and the HIP kernel against both (-m gpu)."""
import os

import numpy as np
import pytest

from oracle import affine_oracle as A

CASES = np.load(os.path.join(os.path.dirname(__file__), "golden", "affine_cases.npz"))
NAMES = sorted({k.split("__")[0] for k in CASES.files})


def oracle_with_fixture_inverse(name):
    """The fixture's own inverse matrix (pinv differs between LAPACK builds in its last bits)."""
    img, tmat, target = CASES[name + "__img"], CASES[name + "__tmat"], tuple(CASES[name + "__target"])
    padded = A.pad_to_shape(img, target)
    if np.array_equal(tmat, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])):
        return padded
    return A.warp_with_inverse(padded, CASES[name + "__inv"]).astype(img.dtype)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_real_skimage(name):
    out = oracle_with_fixture_inverse(name)
    ref = CASES[name + "__out"]
    assert out.dtype == ref.dtype and out.shape == ref.shape
    if ref.dtype == np.float32:
        np.testing.assert_allclose(out, ref, rtol=3e-7, atol=1e-4)    # skimage's f32 path is not bit-pinned
    else:
        assert np.array_equal(out, ref)                                # integer dtypes: bit for bit


def test_public_helper_semantics():
    img, tmat, target = CASES["u8_identity_pad__img"], CASES["u8_identity_pad__tmat"], (33, 36)
    out = A.transform_img_with_tmat(img, target, tmat)
    assert out.shape == target and out.sum() == img.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_warp_affine_matches_oracle_bit_for_bit(name):
    import microaligner_amd as ma
    img, tmat, target = CASES[name + "__img"], CASES[name + "__tmat"], tuple(CASES[name + "__target"])
    got = ma.transform_img_with_tmat(img, target, tmat)
    exp = A.transform_img_with_tmat(img, target, tmat)
    assert got.dtype == img.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp)


@pytest.mark.gpu
def test_hip_warp_affine_large_u16():
    import microaligner_amd as ma
    rng = np.random.default_rng(1)
    img = rng.integers(0, 65535, (700, 900)).astype(np.uint16)
    t = np.deg2rad(0.3)
    tmat = np.array([[np.cos(t), -np.sin(t), 12.5], [np.sin(t), np.cos(t), -7.25]])
    assert np.array_equal(ma.transform_img_with_tmat(img, (720, 930), tmat), A.transform_img_with_tmat(img, (720, 930), tmat))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in NAMES if "identity" not in n])
def test_hip_warp_affine_reproduces_real_skimage_fixtures(name, ctx):
    img, target = CASES[name + "__img"], tuple(CASES[name + "__target"])
    padded = np.ascontiguousarray(A.pad_to_shape(img, target))
    got = ctx.warp_affine(ctx.asdevice(padded), CASES[name + "__inv"]).numpy()
    ref = CASES[name + "__out"]
    if ref.dtype == np.float32:
        np.testing.assert_allclose(got, ref, rtol=3e-7, atol=1e-4)
    else:
        assert np.array_equal(got, ref)


# ---- the clip range of images without a finite value -------------------------------------------------------------
# ma_warp_affine takes its clip range from the shared (min, max) reduction, whose final fold starts from (FLT_MAX, -FLT_MAX):
# for a float32 image whose every value is +Inf or NaN it gives lo = FLT_MAX where a fold from +-INFINITY gives +Inf, and
# hi = -FLT_MAX for -Inf or NaN.  The result must not depend on it: from such an image the warp computes nothing but
# +-Inf, NaN and the 0 outside the source, the clip leaves +-Inf and NaN alone under either range, and 0 is outside both.
F32 = np.float32
INF = F32(np.inf)


def degenerate_image(kind, shape):
    img = np.full(shape, {"pos_inf": INF, "neg_inf": -INF, "pos_inf_one_nan": INF, "all_nan": F32(np.nan), "control": F32(0)}[kind], F32)
    if kind == "pos_inf_one_nan":
        img[shape[0] // 2, shape[1] // 2] = np.nan
    if kind == "control":    # finite, 0 outside its range, a single +Inf
        img[...] = (1.5 + np.arange(img.size, dtype=F32) * F32(0.25)).reshape(shape)
        img[shape[0] // 2, shape[1] // 2] = INF
    return img


def degenerate_inverses():
    t = np.deg2rad(0.3)
    rot = lambda dx, dy: A.inverse_matrix(np.array([[np.cos(t), -np.sin(t), dx], [np.sin(t), np.cos(t), dy]]))
    shift = lambda dx, dy: np.array([[1.0, 0.0, dx], [0.0, 1.0, dy], [0.0, 0.0, 1.0]])
    # the rotation plus shift of test_hip_warp_affine_large_u16 (everything of these small images leaves the frame), the
    # same rotation with a shift that keeps them inside, half a pixel along both axes (dc, dr != 0), and half a pixel
    # along x alone (dr == 0: the 0 * Inf products)
    return {"rot_shift": rot(12.5, -7.25), "rot_subpixel": rot(0.5, -0.25), "half_xy": shift(0.5, 0.5), "half_x": shift(0.5, 0.0)}


DEGENERATE = ["pos_inf", "neg_inf", "pos_inf_one_nan", "all_nan"]
DEGENERATE_SHAPES = [(5, 7), (1, 1)]


def nan_ignoring_bounds(img):
    """the rule the GPU states for its (min, max): NaN never taken, +-Inf are values, the fold starts from (+inf, -inf)"""
    return np.fmin.reduce(img.ravel(), initial=np.inf), np.fmax.reduce(img.ravel(), initial=-np.inf)


def oracle_with_bounds(img, inv):
    with np.errstate(invalid="ignore"):
        return A.warp_with_inverse(img, inv, bounds=nan_ignoring_bounds(img))


def same_bits(got, exp):
    """equal as bit patterns, any NaN payload standing for NaN"""
    assert got.dtype == exp.dtype == F32 and got.shape == exp.shape
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(got.view(np.uint32)[~gn], exp.view(np.uint32)[~en])


@pytest.mark.parametrize("shape", DEGENERATE_SHAPES)
@pytest.mark.parametrize("kind", DEGENERATE)
def test_oracle_of_an_image_without_finite_values_holds_only_inf_nan_and_zero(kind, shape):
    img = degenerate_image(kind, shape)
    seen_nan = False
    for name, inv in degenerate_inverses().items():
        out = oracle_with_bounds(img, inv)
        ok = np.isinf(out) | np.isnan(out) | (out == 0)
        assert ok.all(), (name, out[~ok][:4])
        seen_nan |= bool(np.isnan(out).any())
        if name == "half_x" and kind in ("pos_inf", "neg_inf"):
            assert np.isnan(out).any()        # the 0 * Inf products do occur
    assert seen_nan


def test_default_bounds_of_the_oracle_are_the_image_range():
    img = degenerate_image("control", (5, 7))
    inv = degenerate_inverses()["half_xy"]
    assert same_bits(A.warp_with_inverse(img, inv), A.warp_with_inverse(img, inv, bounds=(img.min(), img.max())))
    assert same_bits(A.warp_with_inverse(img, inv), oracle_with_bounds(img, inv))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DEGENERATE_SHAPES)
@pytest.mark.parametrize("kind", DEGENERATE + ["control"])
def test_hip_warp_affine_clip_range_without_finite_values(kind, shape, ctx):
    img = degenerate_image(kind, shape)
    d = ctx.asdevice(img)
    for name, inv in degenerate_inverses().items():
        got = ctx.warp_affine(d, inv).numpy()
        assert same_bits(got, oracle_with_bounds(img, inv)), (kind, shape, name)
