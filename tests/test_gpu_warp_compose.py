"""-m gpu: the one-resampling warp through a 2x3 matrix and a flow (csrc/warp_compose.hip, include/microaligner_compose.h)
against its float64 statement tests/_warp_compose_ref.py, bit for bit (equal NaN masks, equal signed zeros), through
Context.warp_affine_flow, the page driver, Warper.tmat and parallel.align_pairs(single_resample=True); cross-checks against
the merged remap; non-finite values; sides >= 32767 and pages beyond 2^31 elements; and the two reasons for the feature:
label images survive both stages, and one resampling loses less of a band-limited image than two."""
import numpy as np
import pytest

from microaligner_amd import Warper, _lib as L, transform_img_with_tmat
from microaligner_amd.shared_modules.utils import pad_to_shape
from tests._remap_interp_ref import InterpRef
from tests._warp_compose_ref import compose_map, warp_affine_flow
from tests.test_gpu_warp_interp import _mem_available_gb, flow_for, image
from tests.test_nonfinite import bad_flow, same_bits
from tests.test_warp_compose_ref import IDENTITY, rotation

pytestmark = pytest.mark.gpu

MODES = ["nearest", "linear", "cubic", "lanczos4"]
DTYPES = [np.uint8, np.uint16, np.float32]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return InterpRef(tmp_path_factory.mktemp("warp_compose_ref_gpu"))


def matrices(H, W):
    cx, cy = (W - 1) / 2, (H - 1) / 2
    return {"identity": IDENTITY, "translation": np.array([[1.0, 0.0, 3.25], [0.0, 1.0, -7.5]]),
            "rot3": rotation(3, cx, cy), "sim30": rotation(30, cx, cy, 0.97, 2.0, -1.0), "rot90": rotation(90, cx, cy),
            "singular": np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 5.0]])}


# (image (h, w), flow (H, W)): equal shapes, odd padding, 1-px sides, widths that are not multiples of the 64-column tile
GEOMS = [((53, 71), (53, 71)), ((40, 60), (53, 73)), ((1, 1), (1, 1)), ((1, 30), (4, 35)), ((30, 1), (31, 6)),
         ((67, 130), (70, 131)), ((5, 200), (5, 200))]


@pytest.mark.parametrize("mat", list(matrices(1, 1)))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_exact_against_the_statement(ctx, ref, dtype, mode, mat):
    for (h, w), (H, W) in GEOMS:
        tmat = matrices(H, W)[mat]
        img = image(h, w, dtype, h * 31 + w)
        flow = flow_for(H, W, H + W, 3.0)
        got = ctx.warp_affine_flow(ctx.asdevice(img), ctx.asdevice(flow), tmat, interpolation=mode).numpy()
        same_bits(got, warp_affine_flow(ref, img, flow, tmat, mode))


@pytest.mark.parametrize("mode", MODES + [0, 1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_checks_against_the_merged_remap(ctx, dtype, mode):
    H, W = 97, 150
    img = image(H, W, dtype, 7)
    flow = flow_for(H, W, 8, 4.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    grid = np.stack([xx, yy], -1)
    # identity, no padding: the generic remap of grid - flow (no tile windows)
    got = ctx.warp_affine_flow(ctx.asdevice(img), ctx.asdevice(flow), IDENTITY, interpolation=mode).numpy()
    same_bits(got, ctx.remap(ctx.asdevice(img), ctx.asdevice(grid - flow), interpolation=mode).numpy())
    # zero flow: the generic remap of the padded image at float32(M.grid)
    small = img[5:-8, 3:-10].copy()
    tmat = rotation(30, W / 2, H / 2, 0.97, 2.0, -1.0)
    zero = np.zeros((H, W, 2), np.float32)
    got = ctx.warp_affine_flow(ctx.asdevice(small), ctx.asdevice(zero), tmat, interpolation=mode).numpy()
    padded = np.ascontiguousarray(pad_to_shape(small, (H, W))[0])
    same_bits(got, ctx.remap(ctx.asdevice(padded), ctx.asdevice(compose_map(zero, tmat)), interpolation=mode).numpy())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_values(ctx, ref, dtype, mode):
    H, W = 120, 230
    flow = bad_flow(H, W)
    bad = ~np.isfinite(flow).all(-1) | (np.abs(flow) > 1e11).any(-1)
    img = image(H - 3, W - 4, dtype, 3)
    if dtype == np.float32:
        img[::7, ::5] = np.nan
        img[3::11, 2::9] = np.inf
        img[5::13, 1::17] = -np.inf
    tmat = rotation(3, W / 2, H / 2)
    got = ctx.warp_affine_flow(ctx.asdevice(img), ctx.asdevice(flow), tmat, interpolation=mode).numpy()
    assert np.all(got[bad] == 0) and not np.isnan(got[bad]).any()
    same_bits(got, warp_affine_flow(ref, img, flow, tmat, mode))


@pytest.mark.parametrize("mode", ["linear", "lanczos4"])
@pytest.mark.parametrize("band_bytes", [1, 5000, 32 << 20])
def test_page_driver_matches_the_device_warp(ctx, tmp_path, mode, band_bytes):
    h, w, H, W = 150, 203, 163, 220
    pages = [image(h, w, np.uint16, 40 + k) for k in range(5)]
    flow = ctx.asdevice(flow_for(H, W, 9, 3.0))
    tmat = rotation(30, W / 2, H / 2, 0.97, 2.0, -1.0)
    exp = [ctx.warp_affine_flow(ctx.asdevice(p), flow, tmat, interpolation=mode).numpy() for p in pages]
    old = ctx.get_option(L.MA_OPT_WARP_BAND_BYTES)
    ctx.set_option(L.MA_OPT_WARP_BAND_BYTES, band_bytes)
    try:
        got = ctx.warp_affine_flow_pages(pages, flow, tmat, interpolation=mode)
        mm = np.memmap(tmp_path / "out.raw", dtype=np.uint16, mode="w+", shape=(5, H, W))
        got_mm = ctx.warp_affine_flow_pages(pages, flow, tmat, out=[mm[k] for k in range(5)], interpolation=mode)
    finally:
        ctx.set_option(L.MA_OPT_WARP_BAND_BYTES, old)
    for k in range(5):
        same_bits(got[k], exp[k])
        same_bits(np.asarray(got_mm[k]), exp[k])
        same_bits(np.asarray(mm[k]), exp[k])


def test_warper_paths_agree_and_consume_tmat(ctx):
    from microaligner_amd.device import DeviceArray
    H, W = 4400, 8000                                 # a u16 host page of 70 MB: the page-driver path
    h, w = H - 21, W - 30
    img = np.empty((h, w), np.uint16)
    img[:] = (np.arange(w, dtype=np.uint32)[None, :] * 37 + np.arange(h, dtype=np.uint32)[:, None] * 11).astype(np.uint16)
    assert img.nbytes >= Warper.HOST_BANDED_MIN
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([2.0 * np.sin(yy / 300.0), 1.5 * np.cos(xx / 400.0)], -1).astype(np.float32)
    tmat = rotation(3, W / 2, H / 2, 1.01, 4.5, -2.25)
    dflow = ctx.asdevice(flow)
    exp = ctx.warp_affine_flow(ctx.asdevice(img), dflow, tmat, interpolation="cubic").numpy()
    ctx.forget_host_arrays()
    results = []
    for image_in in (img, ctx.asdevice(img)):
        ww = Warper()
        ww.interpolation, ww.tmat = "cubic", tmat
        ww.image, ww.flow = image_in, flow
        out = ww.warp()
        assert isinstance(out, DeviceArray) == isinstance(image_in, DeviceArray)
        results.append(out.numpy() if isinstance(out, DeviceArray) else out)
        assert ww.tmat is None and len(ww.image) == 0 and len(ww.flow) == 0
    for r in results:
        same_bits(r, exp)
    # a small numpy page: the device path, a numpy result
    small = img[:300, :500].copy()
    ww = Warper()
    ww.tmat, ww.image, ww.flow = tmat, small, flow[:310, :520].copy()
    same_bits(ww.warp(), ctx.warp_affine_flow(ctx.asdevice(small), ctx.asdevice(flow[:310, :520].copy()), tmat).numpy())
    # warp_pages keeps the matrix and the flow
    ww = Warper()
    ww.tmat, ww.flow = tmat, flow[:310, :520].copy()
    a = ww.warp_pages([small, small[::-1].copy()])
    b = ww.warp_pages([small])
    assert ww.tmat is not None and len(ww.flow) == 310
    same_bits(a[0], b[0])
    same_bits(a[0], ctx.warp_affine_flow(ctx.asdevice(small), ctx.asdevice(flow[:310, :520].copy()), tmat).numpy())


def _crop_check(ref, got, img, flow, tmat, mode, rows, cols=None, margin=12):
    """compare the output crop rows x cols with the statement on a crop of the padded source: the crop's integer origin is
    subtracted from the map, exactly (checked), so that cv2.remap's 16-bit coordinates suffice; every tap of the crop's
    samples lies inside the source crop or outside the whole padded source"""
    (H, W), (h, w) = flow.shape[:2], img.shape
    top, left = (H - h) // 2, (W - w) // 2
    (y0, y1), (x0, x1) = rows, cols or (0, W)
    m = compose_map(flow[y0:y1, x0:x1], tmat, y0, x0)
    mx, my = m[..., 0], m[..., 1]
    s0, s1 = max(int(np.floor(my.min())) - margin, 0), min(int(np.ceil(my.max())) + margin, H)
    c0, c1 = max(int(np.floor(mx.min())) - margin, 0), min(int(np.ceil(mx.max())) + margin, W)
    assert s1 - s0 < 32767 and c1 - c0 < 32767
    mc = np.stack([mx - np.float32(c0), my - np.float32(s0)], -1)
    assert np.array_equal(mc + np.array([c0, s0], np.float32), m), "the crop origin does not subtract exactly"
    src = np.zeros((s1 - s0, c1 - c0), img.dtype)
    r0, r1, q0, q1 = max(s0, top), min(s1, top + h), max(c0, left), min(c1, left + w)
    if r1 > r0 and q1 > q0:
        src[r0 - s0:r1 - s0, q0 - c0:q1 - c0] = img[r0 - top:r1 - top, q0 - left:q1 - left]
    same_bits(got[y0:y1, x0:x1], ref.remap(src, mc, mode))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_sides_beyond_32767(ctx, ref, dtype):
    H, W = 40000, 512
    img = image(H - 7, W, dtype, 5)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([1.5 * np.sin(yy / 50.0), 2.0 * np.cos(xx / 40.0)], -1).astype(np.float32)
    tmat = np.array([[1.0, 0.0, 0.4], [0.0, 1.0, 37.25]])       # carries samples across row 32767
    dimg, dflow = ctx.asdevice(img), ctx.asdevice(flow)
    for mode in MODES:
        got = ctx.warp_affine_flow(dimg, dflow, tmat, interpolation=mode).numpy()
        for rows in [(0, 200), (32700, 32850), (32767 + 30, 32767 + 60), (H - 150, H)]:
            _crop_check(ref, got, img, flow, tmat, mode, rows)


@pytest.mark.skipif(_mem_available_gb() < 64, reason="the 2^31-element case needs >= 64 GB of free host memory")
def test_u8_page_beyond_2_31_elements(ctx, ref):
    H, W = 65537, 32768
    assert H * W > 2 ** 31
    yy = np.arange(H, dtype=np.uint32)[:, None]
    xx = np.arange(W, dtype=np.uint32)[None, :]
    img = np.empty((H - 1, W - 2), np.uint8)
    np.bitwise_xor(yy[:-1] * 7 + 3, xx[:, :-2] * 13, out=img, casting="unsafe")
    flow = np.empty((H, W, 2), np.float32)
    flow[..., 0] = (2.3 + np.sin(xx / 97.0)).astype(np.float32)
    flow[..., 1] = (-1.7 + np.cos(yy / 61.0)).astype(np.float32)
    tmat = np.array([[1.0, 0.0, -3.5], [0.0, 1.0, 10.25]])
    dimg, dflow = ctx.asdevice(img), ctx.asdevice(flow)
    for mode in ["linear", "nearest"]:
        out = ctx.warp_affine_flow(dimg, dflow, tmat, interpolation=mode)
        got = out.numpy()
        out.free()
        for rows in [(0, 40), (40000, 40040), (H - 40, H)]:
            for cols in [(0, 300), (20000, 20300), (W - 300, W)]:
                _crop_check(ref, got, img, flow, tmat, mode, rows, cols)


def _smooth_flow(H, W, amp, seed):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    f = np.stack([gaussian_filter(rng.standard_normal((H, W)), 12) for _ in range(2)], -1)
    return (f / np.abs(f).max() * amp).astype(np.float32)


def test_label_images_survive_both_stages(ctx):
    H, W = 220, 260
    rng = np.random.default_rng(4)
    seeds = rng.uniform(0, [W, H], (70, 2))
    ids = rng.choice(np.arange(1000, 60000), 70, replace=False).astype(np.uint16)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (xx[..., None] - seeds[:, 0]) ** 2 + (yy[..., None] - seeds[:, 1]) ** 2
    labels = ids[np.argmin(d, -1)].astype(np.uint16)
    tmat = rotation(12, W / 2, H / 2, 1.04, 3.0, -2.0)
    flow = _smooth_flow(H, W, 2.5, 5)
    w = Warper()
    w.interpolation, w.tmat, w.image, w.flow = "nearest", tmat, labels, flow
    one = w.warp()
    assert set(np.unique(one)) <= set(ids.tolist()) | {0}
    assert len(set(np.unique(one)) & set(ids.tolist())) > 50
    # today's only route blends neighbouring ids in its bilinear affine stage: ids that exist nowhere in the input
    affine = transform_img_with_tmat(labels, (H, W), tmat)
    w = Warper()
    w.interpolation, w.image, w.flow = "nearest", affine, flow
    two = w.warp()
    assert len(set(np.unique(two)) - set(ids.tolist()) - {0}) > 10


def test_one_resampling_beats_two_on_a_band_limited_image(ctx):
    """RMSE against the analytic image of a sum of cosines (periods 5-12 px) under a 7 degree similarity and a smooth
    2-3 px flow.  The CPU statements of both routes give 5.84 (one resampling, linear) and 10.56 (transform_img_with_tmat's
    bilinear stage, then Warper.warp()): a ratio of 0.553, bounded here at 0.65."""
    H = W = 256
    rng = np.random.default_rng(11)
    P, th, ph, a = rng.uniform(5, 12, 6), rng.uniform(0, np.pi, 6), rng.uniform(0, 2 * np.pi, 6), rng.uniform(20, 60, 6)

    def F(x, y):
        return sum(a[k] * np.cos(2 * np.pi * (x * np.cos(th[k]) + y * np.sin(th[k])) / P[k] + ph[k]) for k in range(6)) + 200.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    mov = F(xx, yy).astype(np.float32)
    c, s = np.cos(np.deg2rad(7)), np.sin(np.deg2rad(7))
    tmat = np.array([[c, -s, W / 2 - c * W / 2 + s * H / 2 + 2.3], [s, c, H / 2 - s * W / 2 - c * H / 2 - 1.7]])
    flow = np.stack([2.5 * np.sin(2 * np.pi * yy / 97 + 0.3), 2.2 * np.cos(2 * np.pi * xx / 83)], -1).astype(np.float32)
    M = np.linalg.pinv(np.append(tmat, [[0, 0, 1]], axis=0))
    qx, qy = xx - flow[..., 0], yy - flow[..., 1]
    sx, sy = M[0, 0] * qx + M[0, 1] * qy + M[0, 2], M[1, 0] * qx + M[1, 1] * qy + M[1, 2]
    truth = F(sx, sy)
    inner = (sx > 6) & (sx < W - 7) & (sy > 6) & (sy < H - 7) & (qx > 6) & (qx < W - 7) & (qy > 6) & (qy < H - 7)
    w = Warper()
    w.tmat, w.image, w.flow = tmat, mov, flow
    one = w.warp()
    w = Warper()
    w.image, w.flow = transform_img_with_tmat(mov, (H, W), tmat), flow
    two = w.warp()
    rmse = [np.sqrt(np.mean((o.astype(np.float64) - truth)[inner] ** 2)) for o in (one, two)]
    assert rmse[0] < 0.65 * rmse[1], rmse


@pytest.mark.parametrize("stream", [False, True])
def test_align_pairs_single_resample(ctx, stream):
    from microaligner_amd import parallel, synthetic
    H, W = 1200, 1300
    ref = synthetic.make_cells(H, W, seed=8)
    th = np.deg2rad(0.5)
    M = np.array([[np.cos(th), -np.sin(th), 11.0], [np.sin(th), np.cos(th), -8.0]])
    mov = ctx.warp_affine_cv(ctx.asdevice(ref), M).numpy()
    pairs = [(ref, mov), (ref, mov[::-1].copy())]
    fp, op = dict(num_pyr_lvl=2, tile_size=500), dict(num_pyr_lvl=2, tile_size=400, overlap=60)
    base = parallel.align_pairs(pairs, fp, op, stream=stream)
    one = parallel.align_pairs(pairs, fp, op, stream=stream, single_resample=True)
    for (img0, t0, f0), (img1, t1, f1), (_, m) in zip(base, one, pairs):
        assert np.array_equal(t0, t1) and np.array_equal(f0, f1)
        w = Warper()
        w.tmat, w.image, w.flow = t1, m, f1
        same_bits(img1, w.warp())
