"""-m gpu: cv2.remap's nearest / cubic / Lanczos-4 modes on the device (csrc/remap_interp.hip) against the CPU restatement
tests/c_ref/remap_interp_ref.c, bit for bit (equal NaN masks, equal signed zeros), through the generic remap (1 - 4
channels), the tiled warp, the page-warp driver and Warper; MA_INTER_LINEAR through the new entry points against the
linear ones; unknown modes."""
import ctypes as C
import os

import numpy as np
import pytest

from microaligner_amd import Warper, _lib as L
from tests._remap_interp_ref import InterpRef
from tests.test_nonfinite import CASES, NAMES, bad_flow, case, same_bits
from tests.test_nonfinite import H as NF_H, W as NF_W, TILE as NF_TILE, OV as NF_OV

pytestmark = pytest.mark.gpu

MODES = ["nearest", "cubic", "lanczos4"]
DTYPES = [np.uint8, np.uint16, np.float32]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return InterpRef(tmp_path_factory.mktemp("remap_interp_ref_gpu"))


def image(h, w, dtype, seed, cn=1):
    rng = np.random.default_rng(seed)
    shape = (h, w) if cn == 1 else (h, w, cn)
    if dtype == np.float32:
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=dtype)


def maps(dh, dw, sh, sw, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:dh, 0:dw].astype(np.float32)
    sub = np.stack([rng.uniform(-4, sw + 4, (dh, dw)), rng.uniform(-4, sh + 4, (dh, dw))], -1).astype(np.float32)
    integer = np.stack([rng.integers(-2, sw + 2, (dh, dw)), rng.integers(-2, sh + 2, (dh, dw))], -1).astype(np.float32)
    half = (integer + np.float32(0.5)).astype(np.float32)
    edge = np.stack([xx * ((sw + 10) / max(dw - 1, 1)) - 5 + 0.37, yy * ((sh + 10) / max(dh - 1, 1)) - 5 + 0.61], -1)
    bad = sub.copy()
    bad[0, 0] = (np.nan, 1.0)
    bad[-1, -1] = (1.0, np.inf)
    bad[dh // 2, :3] = (1e12, -1e12)
    bad[:2, dw // 2] = (40000.0, 3.0)
    return {"subpixel": sub, "integer": integer, "half": half, "edges": edge.astype(np.float32), "bad": bad}


def flow_for(h, w, seed, amp=6.0):
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((h, w, 2)) * amp).astype(np.float32)
    f[::5, ::3] = np.round(f[::5, ::3])        # exact integer maps
    f[1::7, ::4] += np.float32(0.5)            # half pixels
    return f


# ---- generic remap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_remap_equals_the_restatement(ctx, ref, mode, dtype, cn):
    for sh, sw in [(37, 45), (1, 1), (1, 19), (23, 1), (7, 8), (300, 520)]:
        src = image(sh, sw, dtype, sh * 7 + sw + cn, cn)
        dsrc = ctx.asdevice(src)
        for name, m in maps(29, 301, sh, sw, sh + sw).items():
            got = ctx.remap(dsrc, ctx.asdevice(m), interpolation=mode).numpy()
            same_bits(got, ref.remap(src, m, mode))


# ---- tiled warp ------------------------------------------------------------------------------------------------------
# ragged windows, tiles below 64 (window origins divided per lane), untiled, 1-px sides, flows that push taps across the
# window and image edges
GEOMS = [((130, 230), 100, 12, 6.0), ((61, 47), 16, 5, 4.0), ((33, 70), 0, 0, 3.0), ((20, 9), 7, 3, 5.0),
         ((1, 1), 100, 10, 1.0), ((1, 300), 100, 10, 3.0), ((300, 1), 64, 20, 3.0), ((257, 515), 128, 30, 40.0),
         ((100, 700), 200, 0, 6.0), ((5, 1000), 0, 0, 8.0)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", GEOMS, ids=[f"{g[0][0]}x{g[0][1]}_t{g[1]}_o{g[2]}" for g in GEOMS])
def test_warp_equals_the_restatement(ctx, ref, mode, dtype, geom):
    (H, W), tile, ov, amp = geom
    img = image(H, W, dtype, H * 3 + W)
    flow = flow_for(H, W, H + W, amp)
    got = ctx.warp(ctx.asdevice(img), ctx.asdevice(flow), tile, ov, interpolation=mode).numpy()
    same_bits(got, ref.warp(img, flow, tile, ov, mode))


# ---- non-finite images and flows (test_nonfinite.py's cases) --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cubic", "lanczos4"])
@pytest.mark.parametrize("name", NAMES)
def test_non_finite_images(ctx, ref, mode, name):
    img = case(name)
    flow = flow_for(NF_H, NF_W, 5, 3.0)
    got = ctx.warp(ctx.asdevice(img), ctx.asdevice(flow), NF_TILE, NF_OV, interpolation=mode).numpy()
    same_bits(got, ref.warp(img, flow, NF_TILE, NF_OV, mode))
    m = flow_for(NF_H, NF_W, 6, 2.0) + np.stack(np.mgrid[0:NF_H, 0:NF_W][::-1], -1).astype(np.float32)
    same_bits(ctx.remap(ctx.asdevice(img), ctx.asdevice(m), interpolation=mode).numpy(), ref.remap(img, m, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_flows(ctx, ref, mode, dtype):
    img = image(NF_H, NF_W, dtype, 9) if dtype != np.float32 else case("nan_tile_borders")
    f = bad_flow(NF_H, NF_W)
    got = ctx.warp(ctx.asdevice(img), ctx.asdevice(f), NF_TILE, NF_OV, interpolation=mode).numpy()
    same_bits(got, ref.warp(img, f, NF_TILE, NF_OV, mode))


# ---- MA_INTER_LINEAR through the new entry points ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_through_the_new_entry_points_gives_the_linear_bits(ctx, dtype):
    H, W, tile, ov = 130, 230, 100, 12
    img = image(H, W, dtype, 21)
    flow = flow_for(H, W, 22)
    dimg, dflow = ctx.asdevice(img), ctx.asdevice(flow)
    dt = {np.uint8: L.MA_U8, np.uint16: L.MA_U16, np.float32: L.MA_F32}[dtype]
    a, b = ctx.empty((H, W), dtype), ctx.empty((H, W), dtype)
    ctx._run(ctx.lib.ma_warp_tiled, dimg.ptr, dt, H, W, dflow.ptr, tile, ov, a.ptr)
    ctx._run(ctx.lib.ma_warp_tiled_interp, dimg.ptr, dt, H, W, dflow.ptr, tile, ov, b.ptr, L.MA_INTER_LINEAR)
    same_bits(b.numpy(), a.numpy())
    m = maps(40, 50, H, W, 23)["subpixel"]
    dm = ctx.asdevice(m)
    ra, rb = ctx.empty((40, 50), dtype), ctx.empty((40, 50), dtype)
    ctx._run(ctx.lib.ma_remap_bilinear, dimg.ptr, dt, 1, H, W, dm.ptr, 40, 50, ra.ptr)
    ctx._run(ctx.lib.ma_remap_interp, dimg.ptr, dt, 1, H, W, dm.ptr, 40, 50, rb.ptr, L.MA_INTER_LINEAR)
    same_bits(rb.numpy(), ra.numpy())
    pages = [img, image(H, W, dtype, 24)]
    out_lin = [np.empty_like(p) for p in pages]
    out_new = [np.empty_like(p) for p in pages]
    src = (C.c_void_p * 2)(*[p.ctypes.data for p in pages])
    ctx._run(ctx.lib.ma_warp_pages_host, src, (C.c_void_p * 2)(*[o.ctypes.data for o in out_lin]), 2, dt, H, W,
             dflow.ptr, tile, ov)
    ctx._run(ctx.lib.ma_warp_pages_host_interp, src, (C.c_void_p * 2)(*[o.ctypes.data for o in out_new]), 2, dt, H, W,
             dflow.ptr, tile, ov, L.MA_INTER_LINEAR)
    for x, y in zip(out_new, out_lin):
        same_bits(x, y)
    # the Python layer's default is the linear path itself
    same_bits(ctx.warp(dimg, dflow, tile, ov, interpolation="linear").numpy(), a.numpy())
    same_bits(ctx.warp(dimg, dflow, tile, ov, interpolation=1).numpy(), a.numpy())


# ---- Warper -------------------------------------------------------------------------------------------------------------
def test_warper_cubic_is_honoured(ref):
    """Warper.interpolation = "cubic" gives the cubic restatement, which differs from the linear result on this input"""
    H, W = 300, 420
    img = image(H, W, np.uint16, 31)
    flow = flow_for(H, W, 32, 2.5)
    w = Warper()
    w.tile_size, w.overlap = 100, 20
    w.image, w.flow = img, flow
    lin = w.warp()
    w = Warper()
    w.tile_size, w.overlap = 100, 20
    w.interpolation = "cubic"
    w.image, w.flow = img, flow
    cub = w.warp()
    exp = ref.warp(img, flow, 100, 20, "cubic")
    same_bits(cub, exp)
    assert not np.array_equal(cub, lin)
    same_bits(lin, ref.warp(img, flow, 100, 20, "linear"))


@pytest.mark.parametrize("mode", ["nearest", "lanczos4", 2])
def test_warper_host_banded_equals_device_resident(ctx, ref, mode):
    """a page of >= 64 MB goes through the page-warp driver in bands; the same page in HBM through the tiled kernel"""
    H, W, tile, ov = 6000, 6100, 1000, 100
    img = image(H, W, np.uint16, 41)
    assert img.nbytes >= Warper.HOST_BANDED_MIN
    flow = flow_for(H, W, 42, 3.0)
    dflow = ctx.asdevice(flow)
    w = Warper()
    w.interpolation = mode
    w.tile_size, w.overlap = tile, ov
    w.image, w.flow = img, dflow
    banded = w.warp()
    w.image, w.flow = ctx.asdevice(img), dflow
    resident = w.warp().numpy()
    same_bits(banded, resident)
    rows = np.sort(np.random.default_rng(43).choice(H, 24, replace=False))
    rows = np.unique(np.concatenate([rows, [0, 899, 900, 1000, 1099, 1100, H - 1]]))
    m = {2: "cubic"}.get(mode, mode)
    same_bits(resident[rows], ref.warp(img, flow, tile, ov, m, rows=rows))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_warp_pages_matches_one_warp_per_page(ctx, ref, mode, dtype):
    H, W, tile, ov = 230, 310, 40, 9
    pages = [image(H, W, dtype, 50 + k) for k in range(5)]
    flow = flow_for(H, W, 51, 5.0)
    w = Warper()
    w.interpolation = mode
    w.tile_size, w.overlap = tile, ov
    w.flow = flow
    old = ctx.get_option(L.MA_OPT_WARP_BAND_BYTES)
    ctx.set_option(L.MA_OPT_WARP_BAND_BYTES, 1)      # one tile row per band: many bands per page
    try:
        out = w.warp_pages(pages)
    finally:
        ctx.set_option(L.MA_OPT_WARP_BAND_BYTES, old)
    out2 = w.warp_pages(pages)                        # default bands: one band per page here
    for p, o, o2 in zip(pages, out, out2):
        single = ctx.warp(ctx.asdevice(p), w.flow, tile, ov, interpolation=mode).numpy()
        same_bits(o, single)
        same_bits(o2, single)
    same_bits(out[0], ref.warp(pages[0], flow, tile, ov, mode))


# ---- unknown modes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["area", "Cubic", 3, 5, -1, True, None, 2.0])
def test_unknown_modes_raise_value_error(ctx, bad):
    w = Warper()
    w.interpolation = bad
    w.image = np.zeros((10, 10), np.uint8)
    w.flow = np.zeros((10, 10, 2), np.float32)
    with pytest.raises(ValueError):
        w.warp()
    assert w.image.shape == (10, 10)          # nothing was consumed: refused before any device work
    with pytest.raises(ValueError):
        w.warp_pages([np.zeros((10, 10), np.uint8)])
    d = ctx.asdevice(np.zeros((10, 10), np.uint8))
    with pytest.raises(ValueError):
        ctx.remap(d, ctx.asdevice(np.zeros((10, 10, 2), np.float32)), interpolation=bad)
    with pytest.raises(ValueError):
        ctx.warp(d, ctx.asdevice(np.zeros((10, 10, 2), np.float32)), 4, 1, interpolation=bad)


def test_unknown_mode_is_refused_by_the_c_abi(ctx):
    d = ctx.asdevice(np.zeros((10, 10), np.uint8))
    f = ctx.asdevice(np.zeros((10, 10, 2), np.float32))
    out = ctx.empty((10, 10), np.uint8)
    for fn, args in [(ctx.lib.ma_warp_tiled_interp, (d.ptr, L.MA_U8, 10, 10, f.ptr, 4, 1, out.ptr, 3)),
                     (ctx.lib.ma_remap_interp, (d.ptr, L.MA_U8, 1, 10, 10, f.ptr, 10, 10, out.ptr, 5))]:
        with pytest.raises(ValueError):
            ctx._run(fn, *args)
    with pytest.raises(ValueError):   # linear keeps ma_remap_bilinear's channel counts
        ctx._run(ctx.lib.ma_remap_interp, d.ptr, L.MA_U8, 3, 10, 10, f.ptr, 3, 3, out.ptr, L.MA_INTER_LINEAR)


# ---- 64-bit element indices ----------------------------------------------------------------------------------------------
def _mem_available_gb():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


BIG_H, BIG_W = 65537, 32768        # 2^31 + 32768 elements: the kernels' 64-bit index path


@pytest.mark.skipif(_mem_available_gb() < 64, reason="the 2^31-element case needs >= 64 GB of free host memory")
def test_u8_image_beyond_2_31_elements(ctx, ref):
    assert BIG_H * BIG_W > 2 ** 31
    yy = np.arange(BIG_H, dtype=np.uint32)[:, None]
    xx = np.arange(BIG_W, dtype=np.uint32)[None, :]
    img = np.empty((BIG_H, BIG_W), np.uint8)
    np.bitwise_xor(yy * 7 + 3, xx * 13, out=img, casting="unsafe")
    flow = np.empty((BIG_H, BIG_W, 2), np.float32)
    flow[..., 0] = (2.3 + np.sin(xx / 97.0)).astype(np.float32)
    flow[..., 1] = (-1.7 + np.cos(yy / 61.0)).astype(np.float32)
    dimg, dflow = ctx.asdevice(img), ctx.asdevice(flow)
    rng = np.random.default_rng(2 ** 31)
    rows = np.unique(np.concatenate([rng.choice(BIG_H, 12, replace=False), [0, 999, 1000, BIG_H - 2, BIG_H - 1]]))
    for mode in ["cubic", "lanczos4", "nearest"]:
        out = ctx.warp(dimg, dflow, 1000, 100, interpolation=mode)
        got = out.numpy()[rows]
        out.free()
        same_bits(got, ref.warp(img, flow, 1000, 100, mode, rows=rows))
