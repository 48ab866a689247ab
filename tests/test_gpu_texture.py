"""-m gpu: the texture support maps on the device.  ma_texture_maps against the numpy float32 statement of
include/microaligner_texture.h (tests/_texture_ref.py) bit for bit; texture_maps(); the weight in an affine fit; refused
arguments; the plumbing of the new header."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_affine_ref as A  # noqa: E402
import _texture_ref as T  # noqa: E402
from _measured_path import HASH  # noqa: E402
from microaligner_amd import TextureMaps, _lib, fit_flow_affine, texture_maps  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402
from test_gpu_flow_affine import E2E_TOL  # noqa: E402
from test_gpu_flow_invert import same_bits  # noqa: E402
from test_gpu_flow_smooth import SHAPES, taps_of  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "microaligner_texture.h")
DTYPES = [np.uint8, np.uint16, np.float32]
CELLS = (16, 48)
SMALL = [(1, 1), (1, 300), (300, 1), (7, 5)]


def make_image(H, W, dtype, seed=0):
    """noise under a smooth envelope that is exactly 0 in the lower right part: textured, edge and flat pixels"""
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    env = np.clip(1.2 - (x / max(W - 1, 1)) ** 2 - (y / max(H - 1, 1)) ** 2, 0, 1)
    v = 0.5 + 0.5 * env * (0.6 * rng.random((H, W)) + 0.4 * np.cos(x / 3.0) - 0.5)
    if dtype is np.float32:
        return v.astype(F32)
    return np.rint(v * np.iinfo(dtype).max).astype(dtype)


def floor_of(ref):
    """a floor inside the image's own range of eigenvalues, so that the classes all occur where the image allows"""
    for lam in (ref["lam_min"], ref["lam_max"]):
        pos = lam[np.isfinite(lam) & (lam > 0)]
        if pos.size:
            return float(np.median(pos))
    return 1.0


def check(ctx, img, taps, cells_list, floor=None):
    """all outputs together per cell size, and each output alone"""
    floor = floor_of(T.texture_maps_ref(img, taps)) if floor is None else floor
    ref = T.texture_maps_ref(img, taps, floor, cells_list[0])
    d = ctx.asdevice(img)
    planes = ("lam_min", "lam_max", "weight")
    for cells in cells_list:
        got = ctx.texture_maps(d, taps, floor, cells, planes)
        for n in planes:
            assert same_bits(got[n].numpy(), ref[n]), n
        exp = T.cell_counts(ref["classes"], cells)
        assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], exp)
    for n in planes:
        got = ctx.texture_maps(d, taps, floor if n == "weight" else None, None, (n,))
        assert list(got) == [n] and same_bits(got[n].numpy(), ref[n]), n
    got = ctx.texture_maps(d, taps, floor, cells_list[0], ())
    assert list(got) == ["counts"] and np.array_equal(got["counts"], ref["counts"])
    return ref


@pytest.mark.parametrize("r", [1, 7, 49, 128])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_numpy_statement_bit_for_bit(ctx, shape, r):
    """u8, u16 and f32; every output alone and all together; cells (16, 48), one cell, and (1, 1) on the small shapes;
    images smaller than r are among the shapes"""
    taps = taps_of(r)
    assert len(taps) == r + 1
    cells_list = [CELLS, (1000, 1000)] + ([(1, 1)] if shape in SMALL else [])
    for dtype in DTYPES:
        check(ctx, make_image(*shape, dtype), taps, cells_list)


def test_a_large_image(ctx):
    """(2049, 1031): many blocks either way; every class occurs"""
    ref = check(ctx, make_image(2049, 1031, np.uint16), taps_of(21), [(100, 100)])
    assert (ref["counts"].sum((0, 1)) > 0).all()


@pytest.mark.parametrize("scale", [1e-20, 3e-10])
def test_denormal_products_and_sums(ctx, scale):
    """1e-20: the products (about 1e-40) and every sum are denormal, and d * d underflows; 3e-10: the sums are about
    1e-19 and their squares under the root are denormal"""
    img = (make_image(65, 129, np.float32) * F32(scale)).astype(F32)
    taps = taps_of(7)
    ref = check(ctx, img, taps, [CELLS])
    tiny = np.finfo(F32).tiny
    if scale == 1e-20:
        assert 0 < ref["lam_max"].max() < tiny and (ref["lam_min"] > 0).any()
    else:
        assert ref["lam_max"].max() > tiny and 0 < float(ref["lam_max"].max()) ** 2 < tiny


@pytest.mark.parametrize("r", [2, 18])
def test_nan_and_inf_pixels(ctx, r):
    img = make_image(67, 301, np.float32)
    img[20, 40], img[50, 200], img[66, 300] = np.nan, np.inf, -np.inf
    clean = T.texture_maps_ref(make_image(67, 301, np.float32), taps_of(r))
    ref = check(ctx, img, taps_of(r), [CELLS], floor_of(clean))
    bad = ~np.isfinite(ref["lam_min"])
    assert bad[20 - r:20 + r + 1, 40 - r:40 + r + 1].all() and 0 < bad.sum() < bad.size
    assert np.isnan(ref["lam_min"][bad]).all() and not ref["weight"][bad].any() and (ref["classes"][bad] == T.FLAT).all()


# ---- texture_maps() --------------------------------------------------------------------------------------------------------
def test_texture_maps_takes_numpy_and_device_arrays(ctx):
    img = make_image(70, 90, np.uint16)
    ref = T.texture_maps_ref(img, T.window_taps(99))
    maps = texture_maps(img)                                     # winsize = 99: r = 49
    assert isinstance(maps, TextureMaps) and isinstance(maps.lam_min, np.ndarray)
    assert same_bits(maps.lam_min, ref["lam_min"]) and same_bits(maps.lam_max, ref["lam_max"])
    assert maps.weight is None and maps.textured is None and maps.cell_bounds is None
    with pytest.raises(ValueError):
        maps.summary()
    floor = floor_of(ref)
    ref = T.texture_maps_ref(img, T.window_taps(99), floor, (32, 40))
    dmaps = texture_maps(ctx.asdevice(img), floor=floor, cell_size=(32, 40))
    for n in ("lam_min", "lam_max", "weight"):
        assert isinstance(getattr(dmaps, n), DeviceArray) and same_bits(getattr(dmaps, n).numpy(), ref[n])
    hmaps = texture_maps(img, floor=floor, cell_size=(32, 40))
    assert same_bits(hmaps.weight, ref["weight"])
    for m in (dmaps, hmaps):
        for k, n in enumerate(("textured", "edges", "flat")):
            assert isinstance(getattr(m, n), np.ndarray) and np.array_equal(getattr(m, n), ref["counts"][..., k])
        assert m.cell_bounds.shape == (3, 3, 4) and tuple(m.cell_bounds[2, 2]) == (64, 70, 80, 90)
        s = m.summary()
        assert s["pixels"] == 70 * 90 and s["cells"] == 9 and abs(s["textured"] + s["edges"] + s["flat"] - 1) < 1e-12
    # sigma and truncate give smooth_flow's taps
    import _flow_smooth_ref as S
    ref = T.texture_maps_ref(img, S.gaussian_taps(2.0, 2.5))
    assert same_bits(texture_maps(img, sigma=2.0, truncate=2.5).lam_min, ref["lam_min"])
    ref = T.texture_maps_ref(img, T.window_taps(15))
    assert same_bits(texture_maps(img, winsize=15).lam_max, ref["lam_max"])


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_dog_labels_are_the_gates(ctx, dtype):
    img = make_image(120, 150, dtype)
    labels = ctx.dog_u8(ctx.asdevice(img), 5, 9)
    assert labels.dtype == np.uint8
    exp = texture_maps(labels, winsize=15, floor=4.0, cell_size=50)
    got = texture_maps(img, winsize=15, labels="dog", floor=4.0, cell_size=50)
    ref = T.texture_maps_ref(labels.numpy(), T.window_taps(15), 4.0, (50, 50))
    for n in ("lam_min", "lam_max", "weight"):
        assert same_bits(getattr(got, n), getattr(exp, n).numpy()) and same_bits(getattr(got, n), ref[n])
    assert np.array_equal(got.textured, exp.textured) and np.array_equal(got.flat, ref["counts"][..., 2])


# ---- the weight does its job -----------------------------------------------------------------------------------------------
def test_the_weight_keeps_an_affine_fit_off_the_empty_half(ctx):
    """96 x 161, r = 7: noise on columns [0, 64), exactly constant from column 64 on, so that lam_min and the weight are
    exactly 0 from column 64 + r + 1 = 72 on.  The flow is exactly affine up to column 80 and that plus (5, 0) px from
    there on -- 81 of 161 columns.  The weighted fit is the exact matrix within the tolerance of an exactly affine flow;
    the unweighted one is off by more than 1 px."""
    H, W, r = 96, 161, 7
    rng = np.random.default_rng(11)
    img = np.full((H, W), 128, np.uint8)
    img[:, :64] = rng.integers(0, 256, (H, 64))
    f = A.affine_flow((H, W), A.DYADIC_AFFINE)
    f[:, 80:, 0] += F32(5)
    maps = texture_maps(img, winsize=2 * r + 1, floor=1.0)
    assert not maps.weight[:, 64 + r + 1:].any() and not maps.lam_max[:, 64 + r + 1:].any()
    assert maps.weight[:, :56].min() > 0.9
    exact = A.inverse(A.DYADIC_AFFINE)
    dev = float(np.abs(fit_flow_affine(f, weight=maps.weight) - exact).max())
    off = np.abs(fit_flow_affine(f) - exact)
    print(f"weighted fit: {dev:.3g} from the exact matrix; unweighted: {off[:, 2].max():.3g} px in translation")
    assert dev <= E2E_TOL
    assert off[:, 2].max() > 1.0


# ---- refused arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_the_c_entry(ctx):
    H, W, big = 50, 60, (1 << 24) + 1
    img = make_image(H, W, np.uint8)
    d = ctx.asdevice(img)
    lo, hi, wt = (ctx.asdevice(np.full((H, W), 7, F32)) for _ in range(3))
    counts = (C.c_longlong * (4 * 2 * 3))()
    taps = (C.c_float * 4)(0.4, 0.2, 0.1, 0.0)

    def bad_taps(*v):
        return (C.c_float * len(v))(*v)
    ok = dict(img=d.ptr, dtype=0, H=H, W=W, taps=taps, r=3, floor=2.0, lo=lo.ptr, hi=hi.ptr, wt=wt.ptr, ch=16, cw=48, counts=counts)
    tm = lambda **kw: ctx._run(ctx.lib.ma_texture_maps, *dict(ok, **kw).values())     # noqa: E731
    tm()
    assert sum(counts) == H * W
    # floor and the cell size are read only when something needs them
    tm(wt=None, counts=None, floor=float("nan"), ch=0, cw=-3)
    tm(counts=None, ch=0, cw=0)
    tm(lo=None, hi=None, wt=None, ch=1000, cw=1000)
    for kw in (dict(img=None), dict(taps=None), dict(lo=None, hi=None, wt=None, counts=None), dict(H=0), dict(W=0),
               dict(H=-1), dict(H=big), dict(W=big), dict(r=0), dict(r=-1), dict(r=129), dict(dtype=3), dict(dtype=-1),
               dict(taps=bad_taps(0.0, 0.2, 0.1, 0.0)), dict(taps=bad_taps(0.4, -0.2, 0.1, 0.0)),
               dict(taps=bad_taps(0.4, 0.2, float("nan"), 0.0)), dict(taps=bad_taps(0.4, 0.2, 0.1, float("inf"))),
               dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")),
               dict(floor=0.0, counts=None), dict(floor=float("nan"), lo=None, hi=None, wt=None),
               dict(ch=0), dict(cw=0), dict(ch=-1)):
        with pytest.raises(ValueError):
            tm(**kw)
    assert ctx.lib.ma_texture_maps(None, *ok.values()) == _lib.MA_EINVAL
    assert ctx.lib.ma_texture_maps(ctx.handle, *dict(ok, r=200).values()) == _lib.MA_EINVAL
    ctx.sync()
    ref = T.texture_maps_ref(img, np.array(taps[:], F32), 2.0, (16, 48))
    assert same_bits(lo.numpy(), ref["lam_min"]) and same_bits(wt.numpy(), ref["weight"])     # a refused call wrote nothing


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    import microaligner_amd
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ma_[a-z0-9_]+)\s*\(", text)))
    assert names == ["ma_texture_maps"] == sorted(_lib.TEXTURE_SIGNATURES)
    assert hasattr(lib, "ma_texture_maps"), "ma_texture_maps declared in microaligner_texture.h but not exported"
    proto = re.search(r"\bma_texture_maps\s*\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.TEXTURE_SIGNATURES["ma_texture_maps"][1])
    others = [_lib.SIGNATURES, _lib.QC_SIGNATURES, _lib.INTERP_SIGNATURES, _lib.COMPOSE_SIGNATURES, _lib.FLOWCOMPOSE_SIGNATURES,
              _lib.FLOWINVERT_SIGNATURES, _lib.RESIDUAL_SIGNATURES, _lib.FLOWGRID_SIGNATURES, _lib.FLOWSMOOTH_SIGNATURES,
              _lib.FLOWAFFINE_SIGNATURES]
    assert not any(set(_lib.TEXTURE_SIGNATURES) & set(t) for t in others)
    assert '#include "microaligner_hip.h"' in open(HEADER).read()
    consts = re.findall(r"#define\s+(MA_[A-Z0-9_]+)\s+(\d+)\b", text)
    assert sorted(n for n, _ in consts) == ["MA_TEXTURE_CLASSES", "MA_TEXTURE_MAX_RADIUS"]
    for name, value in consts:
        assert getattr(_lib, name) == int(value), name
    assert _lib.MA_TEXTURE_MAX_RADIUS == _lib.MA_SMOOTH_MAX_RADIUS       # one check of the taps serves both
    assert {"texture_maps", "TextureMaps"} <= set(microaligner_amd.__all__)


def test_the_source_hash_is_the_parents():
    from microaligner_amd import build
    assert build.source_hash() == HASH == _lib.source_hash()
    assert "texture.hip" in build.SOURCES and "microaligner_texture.h" not in " ".join(build.HEADERS)
    assert [os.path.basename(h) for h in build.SOURCE_HEADERS["texture.hip"]] == ["microaligner_texture.h", "cell_grid.h",
                                                                                  "window_fir.h"]
