"""Texture support maps on the CPU (no GPU): the numpy float32 statement of include/microaligner_texture.h
(tests/_texture_ref.py) against an independent float64 one, the ordering of textured, edge and flat regions, the statement's
identities, and the argument checks of texture_maps_params before any device work."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _texture_ref as T  # noqa: E402

F32, F64 = np.float32, np.float64
DTYPES = [np.uint8, np.uint16, np.float32]
# every operation of the statement is exact with these taps on a uint8 image: products that are multiples of 1/4 below 2^14,
# taps that are powers of two
DYADIC = np.array([0.5, 0.25, 0.125, 0.0625], F32)


def eigenvalues_f64(img, taps):
    from scipy.ndimage import correlate1d
    I = np.asarray(img).astype(F64)
    H, W = I.shape
    xs, ys = np.arange(W), np.arange(H)
    gx = 0.5 * (I[:, np.minimum(xs + 1, W - 1)] - I[:, np.maximum(xs - 1, 0)])
    gy = 0.5 * (I[np.minimum(ys + 1, H - 1), :] - I[np.maximum(ys - 1, 0), :])
    k = np.concatenate([taps[:0:-1], taps]).astype(F64)
    sxx, sxy, syy = (correlate1d(correlate1d(p, k, axis=1, mode="constant"), k, axis=0, mode="constant")
                     for p in (gx * gx, gx * gy, gy * gy))
    h, d = 0.5 * (sxx + syy), 0.5 * (sxx - syy)
    q = np.sqrt(d * d + sxy * sxy)
    return np.maximum(h - q, 0.0), h + q


@pytest.mark.parametrize("r", [3, 21, 49])
@pytest.mark.parametrize("dtype", DTYPES)
def test_statement_against_a_float64_one(dtype, r):
    """The float32 statement against scipy.ndimage.correlate1d(mode="constant") in float64 with the same float32 taps (the
    solver's window of 2r + 1) on the 96 x 160 image of three regions (_texture_ref.three_regions).  Measured
    max(|lam_min32 - lam_min64|, |lam_max32 - lam_max64|) / (2^-24 max(lam_max)):
        uint8:   r = 3: 2.35, r = 21: 7.56, r = 49: 10.10
        uint16:  r = 3: 3.07, r = 21: 6.39, r = 49:  9.92
        float32: r = 3: 2.84, r = 21: 6.20, r = 49:  9.28
    Bound: twice the worst case, rounded up to a power of two: 32 x 2^-24 max(lam_max).
    Medians of lam_min in squared full scale (float32): texture 6.3e-4, 1.5e-3, 1.3e-3 at r = 3, 21, 49; edge 5.3e-6,
    7.7e-6, 7.1e-5; flat 4.7e-6, 7.5e-6, 7.1e-6; lam_max of the edge 1.9e-2, 5.0e-3, 2.5e-3."""
    img, core, full = T.three_regions(dtype)
    taps = T.window_taps(2 * r + 1)
    assert len(taps) == r + 1
    lo, hi = T.eigenvalues(img, taps)
    lo64, hi64 = eigenvalues_f64(img, taps)
    unit = 2.0 ** -24 * float(hi64.max())
    err = max(float(np.abs(lo - lo64).max()), float(np.abs(hi - hi64).max())) / unit
    med = [float(np.median(lo[c])) / full ** 2 for c in core]
    print(f"{np.dtype(dtype)} r = {r}: err = {err:.2f} x 2^-24 max(lam_max); median lam_min texture {med[0]:.2e}, "
          f"edge {med[1]:.2e}, flat {med[2]:.2e}; median lam_max of the edge {float(np.median(hi[core[1]])) / full ** 2:.2e}")
    assert err <= 32


@pytest.mark.parametrize("dtype", DTYPES)
def test_textured_edge_and_flat_regions_land_in_their_classes(dtype):
    """At r = 21 the window (sigma = 6.3 px) fits inside each region.  The noise of 0.4 % of full scale gives gradients of
    variance sigma_n^2 / 2 = 8e-6 of squared full scale, which is what both eigenvalues of the flat part and the smaller one
    of the edge come to; the texture's smaller eigenvalue and the edge's larger one are above 1e-3.  A floor of 1e-4,
    a decade from either group, separates them; the weight follows."""
    img, core, full = T.three_regions(dtype)
    floor = 1e-4 * full ** 2
    m = T.texture_maps_ref(img, T.window_taps(43), floor, (96, 160))
    cls = m["classes"]
    assert (cls[core[0]] == T.TEXTURED).all() and (cls[core[1]] == T.EDGE).all() and (cls[core[2]] == T.FLAT).all()
    assert m["weight"][core[0]].min() > 0.9 and m["weight"][core[1]].max() < 0.1 and m["weight"][core[2]].max() < 0.1
    assert m["counts"].shape == (1, 1, 3) and m["counts"].sum() == img.size
    assert [int((cls == k).sum()) for k in range(3)] == m["counts"][0, 0].tolist()
    # with the solver's own 99-tap window the regions of this small image bleed into each other; the order stays
    lo, hi = T.eigenvalues(img, T.window_taps(99))
    med = [float(np.median(lo[c])) for c in core]
    assert med[0] > 10 * med[1] > 10 * med[2] and float(np.median(hi[core[1]])) > 10 * med[1]


# ---- identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_constant_image_is_exactly_zero_and_flat(dtype):
    img = np.full((40, 70), 37, dtype)
    m = T.texture_maps_ref(img, T.window_taps(15), 1e-6, (16, 48))
    for name in ("lam_min", "lam_max", "weight"):
        assert m[name].dtype == F32 and not m[name].any()
    assert (m["classes"] == T.FLAT).all()
    assert (m["counts"][..., :2] == 0).all() and m["counts"][..., 2].sum() == 40 * 70


@pytest.mark.parametrize("cells", [(16, 48), (1000, 1000), (1, 1), (96, 7)])
def test_counts_sum_to_each_cells_size(cells):
    img, _, full = T.three_regions(np.uint16)
    m = T.texture_maps_ref(img, T.window_taps(15), 1e-4 * full ** 2, cells)
    H, W = img.shape
    ch, cw = min(cells[0], H), min(cells[1], W)
    ys, xs = np.arange(0, H, ch), np.arange(0, W, cw)
    size = (np.minimum(ys + ch, H) - ys)[:, None] * (np.minimum(xs + cw, W) - xs)[None, :]
    assert m["counts"].dtype == np.int64 and m["counts"].shape == (len(ys), len(xs), 3)
    assert np.array_equal(m["counts"].sum(-1), size)
    assert (m["counts"].sum((0, 1)) > 0).all()          # every class occurs in this image
    assert (m["lam_min"] <= m["lam_max"]).all()


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1)])
def test_an_image_of_one_row_or_one_column_has_no_second_direction(shape):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, shape).astype(np.uint16)
    for r in (1, 7, 49):
        lo, hi = T.eigenvalues(img, T.window_taps(2 * r + 1))
        assert not lo.any() and (hi >= 0).all() and (hi.any() == (max(shape) > 1))


def test_transposing_the_image_transposes_the_maps():
    """gx and gy, and Sxx and Syy, change places; h, d * d and Sxy * Sxy do not.  What does not commute in float32 is the
    order of the two passes, which the header fixes (rows, then columns): with the exact arithmetic of dyadic taps on a
    uint8 image the maps come back transposed bit for bit, with Gaussian taps within the bound of
    test_statement_against_a_float64_one on either side of the exact value (measured: 5.1 x 2^-24 max(lam_max))."""
    img, _, _ = T.three_regions(np.uint8)
    imgT = np.ascontiguousarray(img.T)
    a, b = T.texture_maps_ref(img, DYADIC, 50.0, (16, 48)), T.texture_maps_ref(imgT, DYADIC, 50.0, (48, 16))
    for name in ("lam_min", "lam_max", "weight", "classes"):
        assert np.array_equal(a[name].T, b[name]) and a[name].any()
    assert np.array_equal(a["counts"].transpose(1, 0, 2), b["counts"])
    taps = T.window_taps(43)
    for x, y in zip(T.eigenvalues(img, taps), T.eigenvalues(imgT, taps)):
        assert float(np.abs(x.T.astype(F64) - y).max()) <= 64 * 2.0 ** -24 * float(x.max())


def test_non_finite_pixels_spread_by_r_plus_one():
    """a NaN or Inf pixel makes the gradients of its four neighbours non-finite, and the window carries them r further: the
    box of r + 1 around the pixel less its four corners.  lam_min is NaN there; lam_max is NaN or +Inf (Inf + Inf)."""
    img, _, _ = T.three_regions(np.float32)
    img[30, 40], img[70, 120] = np.nan, np.inf
    r = 7
    m = T.texture_maps_ref(img, T.window_taps(2 * r + 1), 1e-4, (16, 48))
    y, x = np.mgrid[0:96, 0:160]
    near = np.zeros((96, 160), bool)
    for py, px in ((30, 40), (70, 120)):
        dy, dx = abs(y - py), abs(x - px)
        near |= (np.maximum(dy, dx) <= r + 1) & ~((dy == r + 1) & (dx == r + 1))
    assert np.isnan(m["lam_min"][near]).all() and not np.isfinite(m["lam_max"][near]).any()
    assert np.isnan(m["lam_max"][30 - r:30 + r, 40 - r:40 + r]).all()
    assert np.isfinite(m["lam_min"][~near]).all() and np.isfinite(m["lam_max"][~near]).all()
    assert not m["weight"][near].any() and (m["classes"][near] == T.FLAT).all()
    assert m["counts"].sum() == img.size


# ---- argument checks -------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_c_entry_raises_before_any_device_work():
    from microaligner_amd.device import texture_maps_params as P
    img = np.zeros((20, 30), np.uint8)
    taps = T.window_taps(7)
    H, W, dtype, t, r, floor, ch, cw, want = P(img, taps)
    assert (H, W, dtype, r, floor, ch, cw, want) == (20, 30, 0, 3, None, None, None, ("lam_min", "lam_max"))
    got = P(img.astype(np.uint16), taps, 2.5, 7, ("weight",))
    assert (got[2], got[5], got[6:]) == (1, 2.5, (7, 7, ("weight",)))
    assert P(img.astype(F32), taps, 1e-3, (4, 1 << 20), ())[6:8] == (4, 1 << 20)

    from microaligner_amd import device
    big = object.__new__(device.DeviceArray)      # sides are checked on the shape alone
    for bad in (dict(img=None), dict(img=[[1, 2]]), dict(img=np.zeros((4, 5, 2), np.uint8)), dict(img=np.zeros(7, np.uint8)),
                dict(img=np.zeros((0, 5), np.uint8)), dict(img=np.zeros((5, 0), F32)), dict(img=np.zeros((4, 5), F64)),
                dict(img=np.zeros((4, 5), np.int16)), dict(img=np.zeros((4, 5), bool)),
                dict(taps=None), dict(taps=list(taps)), dict(taps=taps.astype(F64)), dict(taps=taps[:1]),
                dict(taps=np.ones(130, F32)), dict(taps=np.zeros(4, F32)), dict(taps=-taps),
                dict(taps=np.array([0.5, np.nan], F32)), dict(taps=np.array([0.5, np.inf], F32)),
                dict(taps=np.array([0.0, 0.5], F32)), dict(taps=taps.reshape(2, 2)),
                dict(want=()), dict(want=("lam_min", "lam_min")), dict(want=("lam",)), dict(want="lam_min"),
                dict(want=("weight",)), dict(cell_size=8), dict(want=(), cell_size=8),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=1e-50),
                dict(floor=1e40), dict(floor="1"), dict(floor=True),
                dict(floor=1.0, cell_size=0), dict(floor=1.0, cell_size=(4, 0)), dict(floor=1.0, cell_size=(-1, 4)),
                dict(floor=1.0, cell_size=2.5), dict(floor=1.0, cell_size=(1, 2, 3))):
        with pytest.raises(ValueError):
            P(**dict(dict(img=img, taps=taps), **bad))
    for shape in (((1 << 24) + 1, 2), (2, (1 << 24) + 1)):
        big.shape, big.dtype = shape, np.dtype(np.uint8)
        with pytest.raises(ValueError):
            P(big, taps)
    big.shape = (1 << 24, 1 << 24)
    assert P(big, taps)[:2] == (1 << 24, 1 << 24)
    big.ptr = big.ctx = None             # nothing for __del__ to free


def test_texture_maps_refuses_its_own_arguments_before_any_device_work(monkeypatch):
    from microaligner_amd.shared_modules import texture
    monkeypatch.setattr(texture, "get_context", lambda: pytest.fail("a refused call reached the device"))
    img = np.zeros((20, 30), np.uint8)
    for bad in (dict(winsize=1), dict(winsize=259), dict(winsize=99.0), dict(winsize=True), dict(sigma=0.0),
                dict(sigma=-1.0), dict(sigma=50.0), dict(sigma=2.0, truncate=0.0), dict(sigma="2"), dict(labels="u8"),
                dict(labels=1), dict(cell_size=8), dict(floor=0.0), dict(floor=1.0, cell_size=0)):
        with pytest.raises(ValueError):
            texture.texture_maps(img, **bad)
    with pytest.raises(ValueError):
        texture.texture_maps(np.zeros((4, 5), F64))
    assert len(texture.window_taps(99)) == 50 and len(texture.window_taps(257)) == 129 and len(texture.window_taps(2)) == 2
    assert np.array_equal(texture.window_taps(99), T.window_taps(99))
