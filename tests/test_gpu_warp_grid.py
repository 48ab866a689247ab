"""-m gpu: the warp from a grid flow (ma_warp_affine_grid, include/microaligner_flowgrid.h).  Its definition is the dense
one-resampling warp (microaligner_compose.h, held to its own float64 statement by test_gpu_warp_compose.py) applied to the
expanded grid, bit for bit: all four interpolation modes and three dtypes, the page driver with bands that start and end
inside a grid cell, Warper's routing, and one image of more than 2^31 pixels, for which no dense flow is ever built."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_grid_ref as G  # noqa: E402
from microaligner_amd import FlowGrid, Warper, _lib as L  # noqa: E402
from microaligner_amd.device import DeviceArray  # noqa: E402
from tests._remap_interp_ref import InterpRef  # noqa: E402
from tests.test_gpu_warp_interp import _mem_available_gb, image  # noqa: E402
from tests.test_nonfinite import same_bits  # noqa: E402
from tests.test_warp_compose_ref import IDENTITY, rotation  # noqa: E402
from tests._warp_compose_ref import compose_map  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["nearest", "linear", "cubic", "lanczos4"]
DTYPES = [np.uint8, np.uint16, np.float32]
SIZES = [(65, 130), (257, 300)]      # one and more than one block along x and y, neither a multiple of the tile
STRIDES = [1, 3, 8, 300]


def cases(H, W):
    """(image shape, tmat): the identity without a matrix, a 7 degree similarity of a padded image, a 90 degree rotation"""
    cx, cy = (W - 1) / 2, (H - 1) / 2
    return [((H, W), None), ((H, W), IDENTITY), ((H - 5, W - 8), rotation(7, cx, cy, 0.98, 1.5, -2.0)),
            ((H, W), rotation(90, cx, cy))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_warp_from_a_grid_is_the_dense_warp_of_its_expansion(ctx, dtype, mode):
    for H, W in SIZES:
        f = G.smooth_flow((H, W), H + W, amp=5.0)
        d_f = ctx.asdevice(f)
        for s in STRIDES:
            grid = ctx.flow_grid_sample(d_f, s)
            dense = ctx.flow_grid_expand(grid)
            for (h, w), tmat in cases(H, W):
                img = ctx.asdevice(image(h, w, dtype, h * 3 + w + s))
                got = ctx.warp_affine_grid(img, grid, tmat, interpolation=mode).numpy()
                exp = ctx.warp_affine_flow(img, dense, IDENTITY if tmat is None else tmat, interpolation=mode).numpy()
                same_bits(got, exp)
                assert got.any()
                if s == 1:      # the grid is the flow
                    same_bits(got, ctx.warp_affine_flow(img, d_f, IDENTITY if tmat is None else tmat, interpolation=mode).numpy())


@pytest.mark.parametrize("mode", ["nearest", "linear", "cubic"])
def test_non_finite_nodes_reach_the_warp_as_the_expansion_says(ctx, mode):
    H, W, s = 65, 130, 8
    nodes = G.poison(G.sample_ref(G.smooth_flow((H, W), 3), s), 4, 3)
    grid = FlowGrid(nodes, s, (H, W))
    e = G.expand_ref(nodes, (H, W), s)
    img = ctx.asdevice(image(H, W, np.float32, 5))
    got = ctx.warp_affine_grid(img, grid, interpolation=mode).numpy()
    same_bits(got, ctx.warp_affine_flow(img, ctx.asdevice(e), IDENTITY, interpolation=mode).numpy())
    bad = ~np.isfinite(e).all(-1)
    assert bad.sum() >= s * s and np.all(got[bad] == 0)


@pytest.mark.parametrize("mode", ["linear", "lanczos4"])
def test_page_driver_with_bands_inside_a_cell(ctx, tmp_path, mode):
    """bands of 5 rows at stride 7: a band starts and ends inside a grid cell, and is narrower than the kernel's tile"""
    (h, w), (H, W), s = (60, 120), (65, 130), 7
    pages = [image(h, w, np.uint16, 60 + k) for k in range(3)]
    grid = ctx.flow_grid_sample(ctx.asdevice(G.smooth_flow((H, W), 6, amp=4.0)), s)
    tmat = rotation(7, W / 2, H / 2, 0.98, 1.5, -2.0)
    exp = [ctx.warp_affine_grid(ctx.asdevice(p), grid, tmat, interpolation=mode).numpy() for p in pages]
    old = ctx.get_option(L.MA_OPT_WARP_BAND_BYTES)
    ctx.set_option(L.MA_OPT_WARP_BAND_BYTES, 5 * W * 2)
    try:
        got = ctx.warp_affine_grid_pages(pages, grid, tmat, interpolation=mode)
        mm = np.memmap(tmp_path / "out.raw", dtype=np.uint16, mode="w+", shape=(3, H, W))
        ctx.warp_affine_grid_pages(pages, FlowGrid(grid.nodes.numpy(), s, (H, W)), tmat, out=[mm[k] for k in range(3)],
                                   interpolation=mode)
    finally:
        ctx.set_option(L.MA_OPT_WARP_BAND_BYTES, old)
    for k in range(3):
        same_bits(got[k], exp[k])
        same_bits(np.asarray(mm[k]), exp[k])


def test_warper_routes_a_grid_and_keeps_it(ctx):
    H, W, s = 257, 300, 8
    f = G.smooth_flow((H, W), 7, amp=4.0)
    nodes = G.sample_ref(f, s)
    img = image(H, W, np.uint16, 8)
    small = image(H - 5, W - 8, np.uint16, 9)
    tmat = rotation(7, W / 2, H / 2, 0.98, 1.5, -2.0)
    grid = FlowGrid(nodes, s, (H, W))
    for im, tm, mode in ((img, None, "linear"), (small, tmat, "nearest")):
        exp = ctx.warp_affine_grid(ctx.asdevice(im), grid, tm, interpolation=mode).numpy()
        w = Warper()
        w.image, w.flow, w.tmat, w.interpolation = im, FlowGrid(nodes, s, (H, W)), tm, mode
        got = w.warp()
        assert isinstance(got, np.ndarray) and len(w.image) == 0 and len(w.flow) == 0 and w.tmat is None
        same_bits(got, exp)
        w.image, w.flow, w.tmat = ctx.asdevice(im), FlowGrid(nodes, s, (H, W)), tm
        got = w.warp()
        assert isinstance(got, DeviceArray)
        same_bits(got.numpy(), exp)
        w.flow, w.tmat = FlowGrid(nodes, s, (H, W)), tm
        pages = w.warp_pages([im, im[::-1]])
        same_bits(pages[0], exp)
        assert isinstance(w.flow, FlowGrid) and isinstance(w.flow.nodes, DeviceArray) and w.flow.stride == s
        same_bits(w.warp_pages([im])[0], exp)           # from the resident nodes
    # the whole-image warp, not the tiled one: without tmat the image has the grid's shape
    w = Warper()
    w.image, w.flow = small, grid
    with pytest.raises(ValueError, match="grid's shape"):
        w.warp()
    w.image, w.interpolation = img, "quadratic"
    with pytest.raises(ValueError):
        w.warp()


class _ExpandedCrop:
    """the expanded flow of a grid too large to expand: crops of it, from the statement"""

    def __init__(self, nodes, shape, s):
        self.nodes, self.shape, self.s = nodes, shape + (2,), s

    def __getitem__(self, key):
        rows, cols = key
        return G.expand_ref(self.nodes, self.shape[:2], self.s, rows, cols)


def _crop_check(ref, got, img, flow, mode, rows, cols, margin=12):
    """Compare the output crop rows x cols of an identity-matrix, unpadded warp with the statement on a crop of the source.
    The crop's integer origin is subtracted from the map, exactly (checked), so that cv2.remap's 16-bit coordinates suffice.
    The origin is even in x and in y: nearest rounds the coordinate itself half to even, and beyond 2^15 a float32
    coordinate is a multiple of 2^-8 or coarser, so exact halves are common (about one pixel in 256); an odd origin would
    turn each of them the other way.  Linear rounds 32 times the coordinate, which any integer origin leaves in place."""
    H, W = flow.shape[:2]
    assert img.shape == (H, W)
    (y0, y1), (x0, x1) = rows, cols
    m = compose_map(flow[y0:y1, x0:x1], IDENTITY, y0, x0)
    mx, my = m[..., 0], m[..., 1]
    s0, s1 = max(int(np.floor(my.min())) - margin, 0) & ~1, min(int(np.ceil(my.max())) + margin, H)
    c0, c1 = max(int(np.floor(mx.min())) - margin, 0) & ~1, min(int(np.ceil(mx.max())) + margin, W)
    assert s1 - s0 < 32767 and c1 - c0 < 32767
    mc = np.stack([mx - np.float32(c0), my - np.float32(s0)], -1)
    assert np.array_equal(mc + np.array([c0, s0], np.float32), m), "the crop origin does not subtract exactly"
    same_bits(got[y0:y1, x0:x1], ref.remap(np.ascontiguousarray(img[s0:s1, c0:c1]), mc, mode))


@pytest.mark.skipif(_mem_available_gb() < 64, reason="the 2^31-pixel case needs >= 64 GB of free host memory")
def test_u8_page_beyond_2_31_pixels_from_a_grid(ctx, tmp_path_factory):
    """2 GiB in, 2 GiB out and 4 MB of nodes: the 64-bit index path of the grid instantiations"""
    H, W, s = 32769, 65537, 64
    assert H * W > 2 ** 31
    rng = np.random.default_rng(21)
    img = np.empty((H, W), np.uint8)
    for y in range(0, H, 2048):
        img[y:y + 2048] = rng.integers(0, 256, img[y:y + 2048].shape, dtype=np.uint8)
    gh, gw = G.grid_nodes(H, s), G.grid_nodes(W, s)
    jj, ii = np.mgrid[0:gh, 0:gw].astype(np.float64)
    nodes = np.stack([2.3 + 3 * np.sin(ii / 9.0) * np.cos(jj / 7.0), -1.7 + 2 * np.cos(ii / 5.0 + jj / 11.0)], -1).astype(np.float32)
    grid = FlowGrid(nodes, s, (H, W))
    ref = InterpRef(tmp_path_factory.mktemp("warp_grid_ref_gpu"))
    lazy = _ExpandedCrop(nodes, (H, W), s)
    d_img = ctx.asdevice(img)
    pick = np.random.default_rng(22)
    for mode in ["linear", "nearest"]:
        out = ctx.warp_affine_grid(d_img, grid, interpolation=mode)
        got = out.numpy()
        out.free()
        starts = [0, H - 40] + [int(v) for v in pick.integers(40, H - 80, 3)]
        for y0 in starts:
            for x0 in (0, int(pick.integers(300, W - 600)), W - 300):
                _crop_check(ref, got, img, lazy, mode, (y0, y0 + 40), (x0, x0 + 300))
        del got
