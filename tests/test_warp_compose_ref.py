"""CPU: the float64 statement of the one-resampling warp's map (tests/_warp_compose_ref.py), the argument checks of
Warper.tmat / Context.warp_affine_flow before any device work, and the C-ABI of include/microaligner_compose.h against the
built library and _lib.COMPOSE_SIGNATURES."""
import os
import re

import numpy as np
import pytest

from microaligner_amd import Warper
from microaligner_amd.device import affine_flow_params
from tests._remap_interp_ref import InterpRef
from tests._warp_compose_ref import compose_map, matrix, warp_affine_flow
from tests.test_gpu_warp_interp import flow_for, image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_compose.h")
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def rotation(deg, cx, cy, scale=1.0, tx=0.0, ty=0.0):
    a = np.deg2rad(deg)
    c, s = scale * np.cos(a), scale * np.sin(a)
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty]])


def test_identity_map_is_the_float32_difference():
    flow = flow_for(37, 53, 1)
    m = compose_map(flow, IDENTITY)
    yy, xx = np.mgrid[0:37, 0:53].astype(np.float32)
    assert np.array_equal(m.view(np.uint32), np.stack([xx - flow[..., 0], yy - flow[..., 1]], -1).view(np.uint32))


@pytest.mark.parametrize("t", [(3, -7), (12, 5), (-40, 1)])
def test_integer_translation_is_an_exact_shift(tmp_path, t):
    H, W = 41, 67
    tmat = np.array([[1.0, 0.0, t[0]], [0.0, 1.0, t[1]]])
    m = compose_map(np.zeros((H, W, 2), np.float32), tmat)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    # pinv is not exact, the map lies within 1e-12 of the integers: its 1/32-px quantisation is the shift itself
    assert np.abs(m[..., 0] - (xx - t[0])).max() < 1e-12 and np.abs(m[..., 1] - (yy - t[1])).max() < 1e-12
    assert np.array_equal(np.rint(m * 32).astype(np.int64), np.stack([xx - t[0], yy - t[1]], -1).astype(np.int64) * 32)
    ref = InterpRef(tmp_path)
    img = image(H, W, np.uint16, 5)
    exp = np.zeros_like(img)
    exp[max(t[1], 0):H + min(t[1], 0), max(t[0], 0):W + min(t[0], 0)] = \
        img[max(-t[1], 0):H + min(-t[1], 0), max(-t[0], 0):W + min(-t[0], 0)]
    for mode in ("nearest", "linear"):
        assert np.array_equal(warp_affine_flow(ref, img, np.zeros((H, W, 2), np.float32), tmat, mode), exp)


@pytest.mark.parametrize("tmat", [rotation(3, 30, 20), rotation(30, 26, 18, 0.97, 3.25, -7.5), rotation(90, 31, 19)],
                         ids=["rot3", "sim30", "rot90"])
def test_map_agrees_with_an_independent_float64_evaluation(tmat):
    flow = flow_for(40, 61, 3)
    m = compose_map(flow, tmat)
    # independently: the exact inverse of the 3x3 matrix applied as a matrix product to homogeneous points
    inv = np.linalg.inv(np.append(tmat, [[0, 0, 1]], axis=0))
    yy, xx = np.mgrid[0:40, 0:61].astype(np.float64)
    q = np.stack([xx - flow[..., 0], yy - flow[..., 1], np.ones_like(xx)], -1)
    e = (q @ inv.T)[..., :2]
    ulp = np.spacing(np.abs(e).astype(np.float32))
    assert np.all(np.abs(m.astype(np.float64) - e) <= ulp)


def test_matrix_is_the_pinv_of_transform_img_with_tmat():
    tmat = rotation(30, 26, 18, 0.97)
    assert np.array_equal(matrix(tmat), np.linalg.pinv(np.append(tmat, [[0, 0, 1]], axis=0)))
    _, m, left, top = affine_flow_params((30, 41), np.uint8, (35, 50, 2), np.float32, tmat)
    assert np.array_equal(m, matrix(tmat)[:2].ravel()) and (left, top) == (4, 2)


@pytest.fixture
def no_device(monkeypatch):
    import microaligner_amd.optflow_reg.warper as wmod

    def refuse(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(wmod, "get_context", refuse)


@pytest.mark.parametrize("tmat", [np.eye(3), np.eye(2), [[1, 0, np.nan], [0, 1, 0]], [[1, 0, np.inf], [0, 1, 0]], "x",
                                  [[1, 0, 0], [0, 1]]], ids=["3x3", "2x2", "nan", "inf", "str", "ragged"])
def test_bad_tmat_raises_before_device_work(no_device, tmat):
    w = Warper()
    w.image, w.flow, w.tmat = np.zeros((8, 9), np.uint16), np.zeros((8, 9, 2), np.float32), tmat
    with pytest.raises(ValueError):
        w.warp()
    w.tmat = tmat
    with pytest.raises(ValueError):
        w.warp_pages([np.zeros((8, 9), np.uint16)])


@pytest.mark.parametrize("shape", [(9, 9), (8, 10), (0, 5)])
def test_image_larger_than_the_flow_raises_before_device_work(no_device, shape):
    w = Warper()
    w.image, w.flow, w.tmat = np.zeros(shape, np.uint8), np.zeros((8, 9, 2), np.float32), IDENTITY
    with pytest.raises(ValueError):
        w.warp()


@pytest.mark.parametrize("mode", ["bilinear", 3, 5, True, None])
def test_unknown_mode_raises_before_device_work(no_device, mode):
    w = Warper()
    w.image, w.flow, w.tmat, w.interpolation = np.zeros((8, 9), np.uint8), np.zeros((8, 9, 2), np.float32), IDENTITY, mode
    with pytest.raises(ValueError):
        w.warp()
    with pytest.raises(ValueError):
        affine_flow_params((8, 9), np.uint8, (8, 9, 2), np.float32, IDENTITY, mode)


def test_unsupported_dtype_and_flow_raise_before_device_work(no_device):
    w = Warper()
    w.image, w.flow, w.tmat = np.zeros((8, 9), np.int32), np.zeros((8, 9, 2), np.float32), IDENTITY
    with pytest.raises(ValueError):
        w.warp()
    w.image, w.flow, w.tmat = np.zeros((8, 9), np.uint8), np.zeros((8, 9, 2), np.float64), IDENTITY
    with pytest.raises(ValueError):
        w.warp()


def test_header_exports_and_bindings_agree():
    from microaligner_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_warp_affine_flow", "ma_warp_affine_flow_pages_host"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
    assert sorted(_lib.COMPOSE_SIGNATURES) == names
    assert not set(names) & set(_lib.SIGNATURES)
    # argument counts of the prototypes
    for n in names:
        proto = re.search(r"\b" + n + r"\s*\((.*?)\);", text, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.COMPOSE_SIGNATURES[n][1]), n
