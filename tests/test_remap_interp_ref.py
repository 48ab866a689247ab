"""CPU checks of tests/c_ref/remap_interp_ref.c, the restatement of cv2.remap's nearest / linear / cubic / Lanczos-4 modes
that the GPU kernels of csrc/remap_interp.hip are held to bit for bit (tests/test_gpu_warp_interp.py).

- linear mode: the restatement equals the oracle's remap and tiled warp bit for bit (its quantisation, windows and
  borders are the linear path's);
- cubic and Lanczos-4: within a stated tolerance of an independent float64 statement written from the kernels'
  formulas (Keys' cubic with a = -0.75, the normalised Lanczos window of radius 4), over random subpixel maps, maps at
  exact integers and maps that cross source and window edges;
- the weight tables: 1-D rows sum to 1 within float rounding, every 15-bit 2-D entry sums to 2^15;
- nearest rounds half to even."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import register_oracle as RO
from tests._remap_interp_ref import InterpRef

F32_EPS = float(np.finfo(np.float32).eps)
DTYPES = [np.uint8, np.uint16, np.float32]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return InterpRef(tmp_path_factory.mktemp("remap_interp_ref"))


# ---- float64 statement ------------------------------------------------------------------------------------------------
def keys_cubic(d, a=-0.75):
    d = np.abs(d)
    return np.where(d <= 1, ((a + 2) * d - (a + 3)) * d * d + 1,
                    np.where(d < 2, ((a * d - 5 * a) * d + 8 * a) * d - 4 * a, 0.0))


def lanczos4(d):
    d = np.asarray(d, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = 4.0 * np.sin(np.pi * d) * np.sin(np.pi * d / 4) / (np.pi * d) ** 2
    return np.where(d == 0, 1.0, w)


def weights_1d(mode, frac):
    """(..., N) weights of the taps j = -OFF .. N-1-OFF around the integer part, at fraction frac in [0, 1)"""
    if mode == "cubic":
        j = np.arange(-1, 3)
        return keys_cubic(j - frac[..., None])
    j = np.arange(-3, 5)
    w = lanczos4(j - frac[..., None])
    return w / w.sum(-1, keepdims=True)


def f64_remap(src, map_xy, mode):
    """float64 value of cv2.remap(src, map_xy, None, mode), BORDER_CONSTANT 0 (taps outside the source read 0), with the
    map quantised to 1/32 px as OpenCV does (round half to even); src (h, w) or (h, w, cn)"""
    src = np.asarray(src, np.float64)
    if src.ndim == 2:
        src = src[..., None]
    h, w, cn = src.shape
    q = np.rint(np.clip(map_xy.astype(np.float64), -1e6, 1e6) * 32.0)
    ix, iy = np.floor(q[..., 0] / 32.0), np.floor(q[..., 1] / 32.0)
    fx, fy = q[..., 0] / 32.0 - ix, q[..., 1] / 32.0 - iy
    wx, wy = weights_1d(mode, fx), weights_1d(mode, fy)
    off = 1 if mode == "cubic" else 3
    n = wx.shape[-1]
    acc = np.zeros(map_xy.shape[:2] + (cn,))
    for a in range(n):
        yy = iy.astype(np.int64) - off + a
        for b in range(n):
            xx = ix.astype(np.int64) - off + b
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]
            acc += v * (wy[..., a] * wx[..., b])[..., None]
    return acc


def f64_warp(img, flow, tile, overlap, mode):
    """float64 Warper.warp(): per tile, its zero-padded window of tile + 2 * overlap, the window-local map, f64_remap"""
    H, W = img.shape
    out = np.zeros((H, W))
    P = tile + 2 * overlap
    pad = np.zeros((H + 2 * P, W + 2 * P))
    pad[P:P + H, P:P + W] = img
    for ty in range(-(-H // tile)):
        for tx in range(-(-W // tile)):
            oy, ox = ty * tile - overlap, tx * tile - overlap
            win = pad[P + oy:P + oy + P, P + ox:P + ox + P]
            y0, x0 = ty * tile, tx * tile
            y1, x1 = min(y0 + tile, H), min(x0 + tile, W)
            ly, lx = np.mgrid[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
            f = flow[y0:y1, x0:x1].astype(np.float64)
            m = np.stack([lx - f[..., 0], ly - f[..., 1]], -1).astype(np.float32)
            out[y0:y1, x0:x1] = f64_remap(win, m, mode)[..., 0]
    return out


def check_close(got, exact, dtype, scale):
    """u8 / u16: within 1 LSB of the float64 value (clipped to the type's range); f32: within 8 float32 ulp of the
    value scale (the largest |pixel|)"""
    got = got.astype(np.float64).reshape(exact.shape)
    if dtype == np.float32:
        tol = 8 * F32_EPS * scale
    else:
        exact = np.clip(exact, 0, np.iinfo(dtype).max)
        tol = 1.0
    err = np.abs(got - exact)
    assert err.max() <= tol, f"max error {err.max()} > {tol} at {np.unravel_index(err.argmax(), err.shape)}"


def image(h, w, dtype, seed, cn=1):
    rng = np.random.default_rng(seed)
    shape = (h, w) if cn == 1 else (h, w, cn)
    if dtype == np.float32:
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=dtype)


def maps(dh, dw, sh, sw, seed):
    """name -> (dh, dw, 2) float32 map over an (sh, sw) source"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:dh, 0:dw].astype(np.float32)
    sub = np.stack([rng.uniform(-0.5, sw - 0.5, (dh, dw)), rng.uniform(-0.5, sh - 0.5, (dh, dw))], -1).astype(np.float32)
    integer = np.stack([rng.integers(-2, sw + 2, (dh, dw)), rng.integers(-2, sh + 2, (dh, dw))], -1).astype(np.float32)
    # a smooth map that runs from beyond one edge to beyond the other: taps of every sample cross the borders somewhere
    edge = np.stack([xx * ((sw + 10) / max(dw - 1, 1)) - 5 + 0.37, yy * ((sh + 10) / max(dh - 1, 1)) - 5 + 0.61], -1)
    return {"subpixel": sub, "integer": integer, "edges": edge.astype(np.float32)}


# ---- linear: the restatement is the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cn", [1, 2])
def test_linear_remap_equals_the_oracle(ref, dtype, cn):
    src = image(37, 45, dtype, 1, cn)
    for name, m in maps(29, 33, 37, 45, 2).items():
        np.testing.assert_array_equal(ref.remap(src, m, "linear"), O.remap(src, m), err_msg=name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,tile,ov", [((130, 230), 100, 12), ((61, 47), 16, 5), ((33, 70), 0, 0), ((20, 9), 7, 3)])
def test_linear_warp_equals_the_oracle(ref, dtype, hw, tile, ov):
    H, W = hw
    img = image(H, W, dtype, 3)
    rng = np.random.default_rng(4)
    flow = (rng.standard_normal((H, W, 2)) * 4).astype(np.float32)
    flow[::7, ::5] = np.round(flow[::7, ::5])
    if tile:
        exp = RO.warp(img, flow, tile, ov)
    else:   # one window, the image itself: warper.py's map over the whole image
        yy, xx = np.mgrid[0:H, 0:W]
        exp = O.remap(img, np.stack([xx - flow[..., 0].astype(np.float64), yy - flow[..., 1].astype(np.float64)], -1))
    np.testing.assert_array_equal(ref.warp(img, flow, tile, ov, "linear"), exp)
    rows = [0, H // 2, H - 1]
    np.testing.assert_array_equal(ref.warp(img, flow, tile, ov, "linear", rows=rows), exp[rows])


# ---- cubic / Lanczos-4 against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cubic", "lanczos4"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_remap_is_within_tolerance_of_float64(ref, mode, dtype):
    for sh, sw, cn in [(37, 45, 1), (9, 6, 3), (3, 2, 2), (1, 17, 4)]:
        src = image(sh, sw, dtype, 5 + sh, cn)
        scale = float(np.abs(src.astype(np.float64)).max())
        for name, m in maps(23, 31, sh, sw, 6 + sw).items():
            got = ref.remap(src, m, mode)
            exact = f64_remap(src, m, mode)
            check_close(got, exact, dtype, scale)


@pytest.mark.parametrize("mode", ["cubic", "lanczos4"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,tile,ov", [((130, 230), 100, 12), ((61, 47), 16, 5), ((33, 70), 0, 0)])
def test_warp_is_within_tolerance_of_float64(ref, mode, dtype, hw, tile, ov):
    H, W = hw
    img = image(H, W, dtype, 7)
    rng = np.random.default_rng(8)
    flow = (rng.standard_normal((H, W, 2)) * 6).astype(np.float32)
    flow[::3, ::4] = np.round(flow[::3, ::4])
    got = ref.warp(img, flow, tile, ov, mode)
    exact = f64_warp(img, flow, tile if tile else max(H, W), ov, mode)
    check_close(got, exact, dtype, float(np.abs(img.astype(np.float64)).max()))


def test_integer_maps_copy_the_source_for_f32(ref):
    """at zero fraction cubic weights are (0, 1, 0, 0) exactly; Lanczos-4's are within float rounding of (.., 1, ..)"""
    src = image(20, 30, np.float32, 9)
    yy, xx = np.mgrid[0:20, 0:30].astype(np.float32)
    m = np.stack([xx, yy], -1)
    np.testing.assert_array_equal(ref.remap(src, m, "cubic"), src)
    np.testing.assert_allclose(ref.remap(src, m, "lanczos4"), src, rtol=4 * F32_EPS, atol=0)
    np.testing.assert_array_equal(ref.remap(src, m, "nearest"), src)


# ---- tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cubic", "lanczos4"])
def test_tables(ref, mode):
    t1, tf, ti = ref.tables(mode)
    k = t1.shape[1]
    s = t1.astype(np.float64).sum(1)
    assert np.abs(s - 1).max() <= k * F32_EPS, s
    np.testing.assert_allclose(t1, weights_1d(mode, np.arange(32) / 32.0), atol=4 * F32_EPS)
    assert (ti.astype(np.int64).sum(1) == 32768).all()
    # float 2-D entries are the float products of the 1-D rows: entry fy * 32 + fx, tap (k1, k2) = t1[fy, k1] * t1[fx, k2]
    prod = (t1[:, None, :, None] * t1[None, :, None, :]).reshape(1024, k * k)
    np.testing.assert_array_equal(tf, prod)


# ---- nearest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nearest_rounds_half_to_even(ref, dtype):
    src = image(8, 12, dtype, 10)
    xs = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 10.5, -0.5, 11.5, 2.49999, 2.50001], np.float32)
    ys = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 6.5, 1.0, 7.5, 1.0, 7.49], np.float32)
    m = np.stack([xs, ys], -1)[None]
    got = ref.remap(src, m, "nearest")[0]
    X, Y = np.rint(xs).astype(int), np.rint(ys).astype(int)   # numpy's rint rounds half to even
    assert list(X[:6]) == [0, 2, 2, 4, 4, 10] and list(Y[:6]) == [0, 2, 2, 4, 4, 6]
    ok = (X >= 0) & (X < 12) & (Y >= 0) & (Y < 8)
    exp = np.where(ok, src[np.clip(Y, 0, 7), np.clip(X, 0, 11)], 0).astype(dtype)
    np.testing.assert_array_equal(got, exp)


def test_nearest_warp_picks_window_pixels(ref):
    """nearest through the tiled warp: a pixel of the window (read 0 in its padding or beyond it), never interpolated"""
    H, W, tile, ov = 40, 50, 16, 4
    img = image(H, W, np.uint16, 11)
    rng = np.random.default_rng(12)
    flow = (rng.standard_normal((H, W, 2)) * 5).astype(np.float32)
    got = ref.warp(img, flow, tile, ov, "nearest")
    exp = f64_warp_nearest(img, flow, tile, ov)
    np.testing.assert_array_equal(got, exp)


def f64_warp_nearest(img, flow, tile, ov):
    H, W = img.shape
    out = np.zeros_like(img)
    P = tile + 2 * ov
    for y in range(H):
        oy = (y // tile) * tile - ov
        for x in range(W):
            ox = (x // tile) * tile - ov
            X = int(np.rint(np.float32(x - ox) - flow[y, x, 0]))
            Y = int(np.rint(np.float32(y - oy) - flow[y, x, 1]))
            if 0 <= X < P and 0 <= Y < P and 0 <= ox + X < W and 0 <= oy + Y < H:
                out[y, x] = img[oy + Y, ox + X]
    return out
