"""-m gpu: the residual shift maps (csrc/residual_shift.hip, include/microaligner_residual.h) against the numpy statement
of the header (tests/_residual_shift_ref.py), bit for bit in every output and in the whole table of scores; invariance
under batching, input kind and repetition; residual_shift() over dog / u8 labels of u8, u16 and f32 images; one 8192^2
grid; and an end-to-end run behind register()."""
import numpy as np
import pytest

from _residual_shift_ref import residual_shift_ref
from test_residual_shift_ref import E2E_CELL, E2E_R, E2E_SEED, E2E_SHAPE, e2e_expected_before

KEYS = ("shift_x", "shift_y", "score", "score0", "at_limit", "valid", "table")


def assert_maps_equal(got, exp, cells=None, what=""):
    """got: dict from Context.residual_shift_grid or a ShiftMaps; exp: dict of the statement."""
    for k in KEYS:
        g = got[k] if isinstance(got, dict) else getattr(got, k)
        e = exp[k]
        if cells is not None:
            g = np.array([g[i, j] for i, j in cells])
            e = np.array([e[i, j] for i, j in cells])
        assert g.shape == e.shape, (what, k, g.shape, e.shape)
        assert np.array_equal(g, e, equal_nan=k not in ("at_limit", "valid")), (what, k, g, e)


def grid(ctx, a, b0, b1, cell, R):
    ch, cw = (cell, cell) if isinstance(cell, int) else cell
    return ctx.residual_shift_grid(ctx.asdevice(a), ctx.asdevice(b0), ctx.asdevice(b1) if b1 is not None else None, ch, cw, R,
                                   table=True)


def check(ctx, a, b0, b1, cell, R, what=""):
    m0, m1 = grid(ctx, a, b0, b1, cell, R)
    e0 = residual_shift_ref(a, b0, cell, R)
    assert_maps_equal(m0, e0, what=what + " b0")
    if b1 is None:
        assert m1 is None
    else:
        assert_maps_equal(m1, residual_shift_ref(a, b1, cell, R), what=what + " b1")
    return m0, m1, e0


def noisy_roll(rng, a, dy, dx, noise=30):
    b = np.roll(a, (dy, dx), axis=(0, 1)).astype(np.int32) + rng.integers(-noise, noise + 1, a.shape)
    return np.clip(b, 0, 255).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 4, 16])
def test_random_labels_ragged_grid(ctx, R):
    rng = np.random.default_rng(21 + R)
    H, W = 333, 517                       # tiles of 128 x 32 px: ragged strips, ragged tiles, a ragged grid
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    b0 = noisy_roll(rng, a, 1, -1 if R == 1 else -3)
    b1 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    m0, m1, e0 = check(ctx, a, b0, b1, (150, 200), R, f"R={R}")
    assert m0["valid"].all() and m0["table"].shape == (3, 3, 2 * R + 1, 2 * R + 1)
    assert (np.rint(m0["shift_x"]) == (-1 if R == 1 else -3)).all() and (np.rint(m0["shift_y"]) == 1).all()
    check(ctx, a, b1, None, (150, 200), R, f"R={R} b1 NULL")
    # without the table the maps are the same
    d = [ctx.asdevice(x) for x in (a, b0, b1)]
    n0, n1 = ctx.residual_shift_grid(d[0], d[1], d[2], 150, 200, R)
    assert n0["table"] is None and n1["table"] is None
    for k in KEYS[:-1]:
        assert np.array_equal(n0[k], m0[k], equal_nan=True) and np.array_equal(n1[k], m1[k], equal_nan=True)


@pytest.mark.gpu
def test_few_grey_levels(ctx):
    rng = np.random.default_rng(30)
    a = (rng.integers(0, 3, (260, 300)) * 100).astype(np.uint8)          # 0, 100, 200: many exact ties in the moments
    b0 = np.roll(a, (0, 2), axis=(0, 1))
    b1 = (rng.integers(0, 2, (260, 300)) * 255).astype(np.uint8)
    m0, _, _ = check(ctx, a, b0, b1, 100, 4, "grey levels")
    assert (np.rint(m0["shift_x"]) == 2).all() and (np.rint(m0["shift_y"]) == 0).all()
    a255 = np.full((70, 90), 255, np.uint8)
    a255[::3, ::5] = 0
    check(ctx, a255, np.roll(a255, (1, 1), axis=(0, 1)), None, 40, 4, "0 / 255")   # the largest products


@pytest.mark.gpu
def test_row_column_and_single_line_grids(ctx):
    rng = np.random.default_rng(31)
    H, W = 150, 261
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    b0, b1 = noisy_roll(rng, a, -1, 2), rng.integers(0, 256, (H, W), dtype=np.uint8)
    for cell, shape in (((1, W), (H, 1)), ((H, 1), (1, W)), ((7, 1), (22, W)), ((1, 40), (H, 7)),
                        ((H, 50), (1, 6)), ((50, W), (3, 1)), ((H, W), (1, 1)), ((1000, 1000), (1, 1))):
        m0, _, _ = check(ctx, a, b0, b1, cell, 2, f"cell {cell}")
        assert m0["shift_x"].shape == shape
    m0, _, _ = check(ctx, a, b0, None, (1, 1), 1, "one pixel per cell")
    assert not m0["valid"].any()                                       # n = 1: va = 0
    # images barely larger than 2R: a domain of one row, one column, one pixel
    for shape, R in (((33, 80), 16), ((80, 33), 16), ((9, 9), 4), ((3, 3), 1), ((34, 35), 16)):
        a2, b2 = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
        check(ctx, a2, b2, None, 20, R, f"shape {shape}")
    # h <= 2R through the C-ABI: no domain, every cell invalid (the Python layer refuses such an image)
    a3 = rng.integers(0, 256, (8, 50), dtype=np.uint8)
    m0, _, _ = check(ctx, a3, a3, None, 10, 4, "h = 2R")
    assert not m0["valid"].any() and np.isnan(m0["table"]).all()


@pytest.mark.gpu
def test_constant_cells(ctx):
    rng = np.random.default_rng(32)
    a = rng.integers(0, 256, (300, 400), dtype=np.uint8)
    b0 = noisy_roll(rng, a, 2, 1)
    b1 = b0.copy()
    a[:100, :100] = 9                        # cell (0, 0): the reference constant on its domain
    b0[:104, 100:204] = 77                   # cell (0, 1): b constant for every shift with dx >= 0
    b0[100:200, :100] = 0                    # cell (1, 0): b constant for dy = 0, dx <= 0 only
    b1[200:296, 100:200] = 255               # cell (2, 1): constant for d = 0 only (the domain without its halo)
    m0, m1, e0 = check(ctx, a, b0, b1, 100, 4, "constant cells")
    assert not m0["valid"][0, 0] and np.isnan(m0["table"][0, 0]).all() and not m1["valid"][0, 0]
    t = m0["table"][0, 1]
    assert np.isnan(t[:, 4:]).all() and np.isfinite(t[:, :4]).all() and m0["valid"][0, 1] and m0["shift_x"][0, 1] < 0
    t = m0["table"][1, 0]
    assert np.isnan(t[4, :5]).all() and np.isfinite(t).sum() == 76 and np.isnan(m0["score0"][1, 0]) and m0["valid"][1, 0]
    t = m1["table"][2, 1]
    assert np.isnan(t[4, 4]) and np.isfinite(t).sum() == 80 and m1["valid"][2, 1]
    assert m0["valid"][2].all() and (m0["shift_x"][2] != 0).all()


@pytest.mark.gpu
def test_results_do_not_depend_on_workspace_limit_inputs_or_repetition(ctx):
    from microaligner_amd import _lib as L
    from microaligner_amd import residual_shift
    rng = np.random.default_rng(33)
    H, W = 700, 900
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    b0 = noisy_roll(rng, a, -2, 3)
    flow = np.zeros((H, W, 2), np.float32)

    def same(x, y):
        for k in KEYS:
            assert np.array_equal(getattr(x, k), getattr(y, k), equal_nan=True), k
            assert np.array_equal(getattr(x.before, k), getattr(y.before, k), equal_nan=True), k

    kw = dict(cell_size=(90, 110), max_shift=4, labels="u8", warped=b0, return_table=True)
    base = residual_shift(a, a, flow, **kw)
    exp = residual_shift_ref(a, b0, (90, 110), 4)
    assert_maps_equal(base, exp, what="u8 labels, warped given")
    assert_maps_equal(base.before, residual_shift_ref(a, a, (90, 110), 4), what="before")
    assert base.shift_x.shape == (8, 9) and base.cell_bounds.shape == (8, 9, 4)
    same(base, residual_shift(a, a, flow, **kw))
    d = {k: ctx.asdevice(v) for k, v in (("a", a), ("flow", flow), ("b0", b0))}
    same(base, residual_shift(d["a"], d["a"], d["flow"], **dict(kw, warped=d["b0"])))
    # the smallest workspace limit there is, 1 MiB: at R = 16 with the table a cell and two images take 69 796 B (3269 u64
    # moments, 1089 + 4 doubles and two flags, each twice), so the 72 cells go through in batches of 15
    kw16 = dict(kw, max_shift=16)
    base16 = residual_shift(a, a, flow, **kw16)
    assert_maps_equal(base16, residual_shift_ref(a, b0, (90, 110), 16), what="R = 16")
    prev = ctx.get_option(L.MA_OPT_WORKSPACE_LIMIT)
    try:
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, 1 << 20)
        small = residual_shift(a, a, flow, **kw16)
    finally:
        ctx.set_option(L.MA_OPT_WORKSPACE_LIMIT, prev)
    same(base16, small)
    # zero flow and no `warped`: the warp returns the image, `after` equals `before`
    z = residual_shift(a, b0, flow, cell_size=(90, 110), max_shift=4, labels="u8", return_table=True)
    assert_maps_equal(z, exp, what="zero flow")
    assert_maps_equal(z.before, exp, what="zero flow, before")
    g = residual_shift(a, b0, None, cell_size=(90, 110), max_shift=4, labels="u8", return_table=True)
    assert_maps_equal(g, exp, what="as given")
    assert g.before is None
    assert residual_shift(a, b0, flow, cell_size=(90, 110), labels="u8", before=False).before is None
    s = base.summary()
    assert s["cells"] == 72 and s["cells_valid"] == 72 and s["worst_cell_bounds"] == tuple(base.cell_bounds[s["worst_cell"]])
    assert s["max"] == base.magnitude.max() and s["median"] <= s["p95"] <= s["max"] and s["before"]["max"] <= 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("labels", ["dog", "u8"])
def test_residual_shift_labels_and_dtypes(ctx, labels, dtype):
    from microaligner_amd import residual_shift, synthetic
    H, W = 420, 404
    ref, mov = synthetic.make_pair(H, W, 6, dtype=dtype)
    rng = np.random.default_rng(34)
    flow = (rng.standard_normal((H, W, 2)) * 0.7).astype(np.float32)
    flow[..., 0] += 3.0
    rs = residual_shift(ref, mov, flow, cell_size=150, max_shift=6, labels=labels, tile_size=200, overlap=30,
                        return_table=True)
    d_ref, d_mov = ctx.asdevice(ref), ctx.asdevice(mov)
    wrp = ctx.warp(d_mov, ctx.asdevice(flow), 200, 30)
    if labels == "dog":
        lab = [ctx.dog_u8(x).numpy() for x in (d_ref, wrp, d_mov)]
    else:
        lab = [(x if x.dtype == np.uint8 else ctx.normalize_minmax_u8(x)).numpy() for x in (d_ref, wrp, d_mov)]
    assert_maps_equal(rs, residual_shift_ref(lab[0], lab[1], 150, 6), what=f"{labels} {np.dtype(dtype)} after")
    assert_maps_equal(rs.before, residual_shift_ref(lab[0], lab[2], 150, 6), what=f"{labels} {np.dtype(dtype)} before")
    assert rs.valid.all() and rs.before.valid.all()


@pytest.mark.gpu
def test_large_grid_8192(ctx):
    """8192^2, cells of 1000 (a 9 x 9 grid, the last row and column 192 px), R = 4, two label images.  Held to the statement
    on the cells (0, 0), (3, 5), (4, 0), (7, 7), (8, 2), (2, 8) and (8, 8): corners, edges, interior and the ragged ones."""
    rng = np.random.default_rng(35)
    H = W = 8192
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    b0 = np.roll(a, (1, -2), axis=(0, 1))
    b0[::7] = rng.integers(0, 256, b0[::7].shape, dtype=np.uint8)
    b1 = np.roll(a, (-3, 4), axis=(0, 1))
    cells = [(0, 0), (3, 5), (4, 0), (7, 7), (8, 2), (2, 8), (8, 8)]
    m0, m1 = grid(ctx, a, b0, b1, 1000, 4)
    assert m0["shift_x"].shape == (9, 9) and m0["valid"].all() and m1["valid"].all()
    assert_maps_equal(m0, residual_shift_ref(a, b0, 1000, 4, cells=cells), cells=cells, what="8192 b0")
    assert_maps_equal(m1, residual_shift_ref(a, b1, 1000, 4, cells=cells), cells=cells, what="8192 b1")
    assert (np.rint(m0["shift_x"]) == -2).all() and (np.rint(m0["shift_y"]) == 1).all()
    assert (m1["shift_x"] == 4.0).all() and (np.rint(m1["shift_y"]) == -3).all() and m1["at_limit"].all()
    assert not m0["at_limit"].any()


@pytest.mark.gpu
def test_end_to_end_after_register(ctx):
    """synthetic.make_pair (u8), register(), residual_shift with R = 6 (E2E_R: the synthetic displacement stays below 5.3 px
    per axis; tests/test_residual_shift_ref.py shows that the statement alone reads it within 0.25 px at this R).

    before: -(cell mean of synthetic.displacement(), which holds GLOBAL_SHIFT) within 0.25 px wherever not at_limit -- the
    minus sign because make_pair gives mov(p) = ref(p + d) and the header's sign is ref(p) ~ mov(p + shift).
    That check runs on the u8 labels, where its premise can be shown without a GPU.  On the dog labels (a band-pass of sigma
    5 / 9 px) the statement itself, on the CPU, is off the cell mean by up to 0.332 px in x (0.179 px in y) at R = 6 and by
    0.330 px at R = 8: the displacement varies by +-2 px inside a cell and the correlation peak of a band-passed texture is
    not the mean of that.  No R makes the statement meet 0.25 px there, so for the dog labels the figures are printed only.
    after: every valid cell at least 64 px from the border has a smaller magnitude than before, with both kinds of labels."""
    from microaligner_amd import OptFlowRegistrator, residual_shift, synthetic
    H, W = E2E_SHAPE
    ref, mov = synthetic.make_pair(H, W, E2E_SEED, dtype=np.uint8)
    reg = OptFlowRegistrator()
    reg.verbose = False
    for k, v in dict(num_pyr_lvl=2, use_full_res_img=True, use_dog=True, tile_size=200, overlap=30).items():
        setattr(reg, k, v)
    reg.ref_img, reg.mov_img = ref, mov
    flow = reg.register()
    ex, ey = e2e_expected_before()
    for labels in ("u8", "dog"):
        rs = residual_shift(ref, mov, flow, cell_size=E2E_CELL, max_shift=E2E_R, labels=labels, tile_size=200, overlap=30)
        b = rs.cell_bounds
        inner = (b[..., 0] >= 64) & (b[..., 1] <= H - 64) & (b[..., 2] >= 64) & (b[..., 3] <= W - 64)
        sel = inner & rs.valid & rs.before.valid
        print(labels, "after", np.round(rs.magnitude, 3).tolist(), "before", np.round(rs.before.magnitude, 3).tolist())
        assert sel.sum() == 2 * 3 and rs.valid.all() and rs.before.valid.all()
        assert (rs.magnitude[sel] < rs.before.magnitude[sel]).all()
        ok = ~rs.before.at_limit
        assert ok.any()
        ea, eb = np.abs(rs.before.shift_x - ex)[ok].max(), np.abs(rs.before.shift_y - ey)[ok].max()
        print(labels, f"before vs synthetic displacement: worst |dx| error {ea:.3f}, |dy| error {eb:.3f} px")
        if labels == "u8":
            assert ea <= 0.25 and eb <= 0.25
        s = rs.summary()
        assert s["cells"] == 20 and s["before"]["median"] > s["median"]
