"""The host decisions about a weight argument, without a device: which kind and which cells the six *_params functions
that take a weight (smooth_flow, median_flow, flow_affine_moments, direct_affine_moments, flow_refine_step,
local_correlation) make of it, and what they refuse; the 2 x 3 matrices of prior, mat and M; the `want` of texture_maps and
local_correlation.  Kinds, cell sizes and the exception type are asserted, not the messages."""
import numpy as np
import pytest

from microaligner_amd import _lib as L
from microaligner_amd import device as D

F32 = np.float32
H, W = 6, 10
NONE, PIXELS, MASK, CELLS = (L.MA_SMOOTH_WEIGHT_NONE, L.MA_SMOOTH_WEIGHT_F32, L.MA_SMOOTH_WEIGHT_U8,
                             L.MA_SMOOTH_WEIGHT_CELLS)
FLOW, IMG, TAPS = np.zeros((H, W, 2), F32), np.zeros((H, W), F32), D.gaussian_taps(1.0)
EYE = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]


# every call -> (kind, (cell_h, cell_w)); the calls without a cell grid give None for it
def smooth(weight, cell_size=None):
    r = D.smooth_flow_params(FLOW, TAPS, weight, cell_size)
    return r[4], r[5:7]


def median(weight, cell_size=None):
    r = D.median_flow_params(FLOW, 2, weight, cell_size)
    return r[3], r[4:6]


def affine(weight, cell_size=None):
    r = D.flow_affine_moments_params(FLOW, weight, cell_size)
    return r[2], r[3:5]


def direct(weight):
    return D.direct_affine_moments_params(IMG, IMG, EYE, weight=weight)[7], None


def refine(weight):
    return D.flow_refine_step_params(IMG, IMG, FLOW, TAPS, 1.0, weight)[6], None


def localcorr(weight):
    return D.local_correlation_params(IMG, IMG, TAPS, 1.0, weight=weight)[7], None


WITH_CELLS = {"smooth": smooth, "median": median, "affine": affine}
PER_PIXEL_ONLY = {"direct": direct, "refine": refine, "localcorr": localcorr}
ALL = {**WITH_CELLS, **PER_PIXEL_ONLY}
NO_CELLS = {"smooth": (1, 1), "median": (1, 1), "affine": (H, W), "direct": None, "refine": None, "localcorr": None}


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("weight, kind", [(None, NONE), (np.ones((H, W), F32), PIXELS), (np.ones((H, W), np.uint8), MASK)],
                         ids=["none", "float32", "uint8"])
def test_per_pixel_kinds(name, weight, kind):
    assert ALL[name](weight) == (kind, NO_CELLS[name])


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("weight", [np.ones((H, W), np.float64), np.ones((W, H), F32), np.ones((H, W, 1), F32),
                                    [[1.0] * W] * H], ids=["float64", "transposed", "3-D", "list"])
def test_refused_weights(name, weight):
    with pytest.raises(ValueError):
        ALL[name](weight)


@pytest.mark.parametrize("name", WITH_CELLS)
def test_per_cell_map(name):
    assert WITH_CELLS[name](np.ones((2, 3), F32), (4, 4)) == (CELLS, (4, 4))
    with pytest.raises(ValueError):
        WITH_CELLS[name](np.ones((2, 3), np.uint8), (4, 4))


@pytest.mark.parametrize("name", PER_PIXEL_ONLY)
def test_per_cell_map_where_none_is_taken(name):
    with pytest.raises(ValueError):
        PER_PIXEL_ONLY[name](np.ones((2, 3), F32))


@pytest.mark.parametrize("name", ["smooth", "median"])
def test_cell_size_belongs_to_a_per_cell_map(name):
    with pytest.raises(ValueError):
        WITH_CELLS[name](np.ones((H, W), F32), (4, 4))
    with pytest.raises(ValueError):
        WITH_CELLS[name](None, (4, 4))


def test_cell_size_is_the_grid_of_the_affine_moments():
    assert affine(np.ones((H, W), F32), (4, 4)) == (PIXELS, (4, 4))
    assert affine(np.ones((H, W), np.uint8), (4, 4)) == (MASK, (4, 4))
    assert affine(None, (4, 4)) == (NONE, (4, 4))


@pytest.mark.parametrize("cell_size", [0, True, (4,), "4"], ids=repr)
def test_refused_cell_sizes(cell_size):
    for name in ("smooth", "median", "affine"):
        with pytest.raises(ValueError):
            WITH_CELLS[name](np.ones((2, 3), F32), cell_size)
    with pytest.raises(ValueError):
        affine(None, cell_size)
    with pytest.raises(ValueError):
        D.texture_maps_params(IMG, TAPS, 1.0, cell_size)
    with pytest.raises(ValueError):
        D.local_correlation_params(IMG, IMG, TAPS, 1.0, cell_size=cell_size)


# ---- the 2 x 3 matrices ----------------------------------------------------------------------------------------------------
MATRIX = {"prior": lambda m: D.flow_affine_moments_params(FLOW, prior=m, clip=1.0)[5],
          "mat": lambda m: D.flow_affine_apply_params(FLOW, m)[2],
          "M": lambda m: D.direct_affine_moments_params(IMG, IMG, m)[4]}


@pytest.mark.parametrize("name", MATRIX)
def test_matrix_2x3(name):
    m = [[1.5, -2.0, 3.25], [4.0, 5.5, -6.0]]
    for given in (m, np.array(m, F32), tuple(map(tuple, m))):
        got = MATRIX[name](given)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (6,) and got.flags.c_contiguous
        assert got.tolist() == [1.5, -2.0, 3.25, 4.0, 5.5, -6.0]
    for bad in (np.ones((3, 2)), [[1.0, 0.0, np.nan], [0.0, 1.0, 0.0]], [[1.0, 0.0, np.inf], [0.0, 1.0, 0.0]], "matrix"):
        with pytest.raises(ValueError):
            MATRIX[name](bad)


# ---- want and the cells of the counts --------------------------------------------------------------------------------------
WANT = {"texture": (lambda want, cell_size=None: D.texture_maps_params(IMG, TAPS, 1.0, cell_size, want)[6:9], "lam_min", "weight"),
        "localcorr": (lambda want, cell_size=None: D.local_correlation_params(IMG, IMG, TAPS, 1.0, cell_size=cell_size,
                                                                             want=want)[11:14], "score", "weight")}


@pytest.mark.parametrize("name", WANT)
def test_want(name):
    call, a, b = WANT[name]
    assert call([a, b]) == (None, None, (a, b))
    assert call((b,), 4) == (4, 4, (b,))
    assert call((), (4, 5)) == (4, 5, ())
    for bad in (a, (a, a), (a, "counts"), (a, 1), ()):
        with pytest.raises(ValueError):
            call(bad)
