"""Cases of the registry: flows."""
import numpy as np

from .registry import F32, F64, SHAPE, _RO, assert_same, case, dev
from .warps import OV, TILE


@case("merge_flows[window shortcuts, cell maxima from the warps, banded, untiled]",
      ("ma_merge_flows_tiled", "ma_merge_flows_tiled_cells", "ma_warp_tiled_flowcells"))
def _(env):
    from test_gpu_primitives import rand_flow
    RO = _RO()
    ctx = env.ctx
    h, w = SHAPE
    f1, f2 = rand_flow(h, w, 1, 3.0), rand_flow(h, w, 2, 2.0)
    f1[:25, :100] = 0                                # flow1 all zero in some windows
    f1[30:, :70] = -np.abs(f1[30:, :70])              # max == 0 only through the zero padding
    f2[35:, 150:] = 0
    f2[3, 5, 1] = np.nan                              # a window that takes the general branch whatever else it holds
    img = np.random.default_rng(1).random((h, w)).astype(F32)
    geoms = [(TILE, OV), (40, 25), (0, 0)]            # cells; tile <= 2 overlap: the banded reduction; one window
    exp = [RO.merge_flows(f1, f2, t, o) if t else RO.merge_two_flows(f1, f2) for t, o in geoms]
    exp.append(exp[0])

    def run():
        got = [ctx.merge_flows(*dev(ctx, f1, f2), t, o).numpy() for t, o in geoms]
        d1, d2, dimg = dev(ctx, f1, f2, img)
        for d in (d1, d2):
            ctx.warp(dimg, d, TILE, OV, minmax=True, flow_cells=True)
        got.append(ctx.merge_flows(d1, d2, TILE, OV).numpy())
        return got
    return run, exp


@case("compose_flows", "ma_compose_flows")
def _(env):
    import _flow_compose_ref as R
    from test_gpu_flow_compose import flows
    ctx = env.ctx
    pairs = [flows(*SHAPE, kind, seed=5) for kind in ("few_px", "hundreds_px", "integers")]
    pairs[0][1][5, 6] = (np.nan, 1.0)
    pairs[0][1][66, 300] = (-np.inf, np.nan)
    exp = [R.compose_flows_ref(a, b) for a, b in pairs]
    return (lambda: [ctx.compose_flows(*dev(ctx, a, b)).numpy() for a, b in pairs]), exp


@case("invert_flow", "ma_invert_flow")
def _(env):
    import _flow_invert_ref as R
    from test_gpu_flow_invert import make_flow
    ctx = env.ctx
    fs = [make_flow(*SHAPE, kind) for kind in ("smooth", "folding", "non_finite")]
    exp = []
    for f in fs:
        e, res, missed, _ = R.invert_flow_ref(f, 25, 1e-3)
        exp.append((e, e, res, missed))

    def run():
        got = []
        for f in fs:
            d = dev(ctx, f)
            out, info = ctx.invert_flow(d, 25, 1e-3, return_info=True)
            got.append((ctx.invert_flow(d, 25, 1e-3).numpy(), out.numpy(), info.residual.numpy(), info.not_converged))
        return got
    return run, exp


@case("transform_points", "ma_transform_points")
def _(env):
    import _flow_invert_ref as R
    from microaligner_amd.device import affine_flow_params
    from test_gpu_flow_invert import TMAT, make_flow, points
    ctx = env.ctx
    H, W = SHAPE
    f = make_flow(H, W, "smooth")
    pts = points(1000, H, W, 5)
    shape = (H - 21, W - 10)
    _, m6, left, top = affine_flow_params(shape, F32, f.shape, f.dtype, TMAT)
    exp = [R.to_moving_ref(pts, f, None, (0, 0)), R.to_reference_ref(pts, f, None, (0, 0), 30, 1e-4)[:3],
           R.to_moving_ref(pts, f, m6, (left, top)), R.to_reference_ref(pts, f, TMAT.ravel(), (left, top), 30, 1e-4)[:3]]
    exp = [(e[0], e[1].astype(bool), e[2].astype(bool)) for e in exp]

    def run():
        d = dev(ctx, f)
        got = []
        for kw in (dict(), dict(tmat=TMAT, image_shape=shape)):
            for direction in ("to_moving", "to_reference"):
                p, info = ctx.transform_points(pts, d, direction, max_iter=30, tol=1e-4, return_info=True, **kw)
                got.append((p, info.converged, info.inside))
        return got
    return run, exp


@case("flow_grid_sample, flow_grid_expand, flow_grid_error, transform_points[grid]",
      ("ma_flow_grid_sample", "ma_flow_grid_expand", "ma_flow_grid_error", "ma_transform_points_grid"))
def _(env):
    import _flow_grid_ref as G
    from microaligner_amd import FlowGrid
    from test_gpu_flow_grid import grid_points
    ctx = env.ctx
    shape, s, cell, tol = (65, 130), 7, (16, 16), 1 / 32
    f = G.poison(G.smooth_flow(shape, 11), 12)
    nodes = G.sample_ref(f, s)
    clean = G.sample_ref(G.smooth_flow(shape, 15, amp=3.0), s)
    pts = grid_points(shape, s, 16)
    mv, rf = G.to_moving_grid_ref(pts, clean, shape, s), G.to_reference_grid_ref(pts, clean, shape, s, None, (0, 0), 30, 1e-4)
    exp = (nodes, G.expand_ref(nodes, shape, s), tuple(G.error_maps_ref(f, nodes, s, cell, tol)),
           (mv[0], mv[1].astype(bool), mv[2].astype(bool)), (rf[0], rf[1].astype(bool), rf[2].astype(bool)))

    def run():
        d = dev(ctx, f)
        grid = ctx.flow_grid_sample(d, s)
        given = FlowGrid(nodes, s, shape)
        pg = FlowGrid(dev(ctx, clean), s, shape)
        a, ia = ctx.transform_points(pts, pg, "to_moving", return_info=True)
        b, ib = ctx.transform_points(pts, pg, "to_reference", max_iter=30, tol=1e-4, return_info=True)
        return (grid.nodes.numpy(), ctx.flow_grid_expand(given).numpy(), tuple(ctx.flow_grid_error(d, given, *cell, tol)),
                (a, ia.converged, ia.inside), (b, ib.converged, ib.inside))
    return run, exp


KINDS = ("none", "f32", "u8", "cells")

for _r in (2, 128):
    for _kind in KINDS:
        def _smooth(r=_r, kind=_kind):
            @case(f"smooth_flow[r={r},{kind}]", "ma_smooth_flow")
            def _(env):
                import _flow_smooth_ref as R
                from test_gpu_flow_smooth import make_flow, make_weight, taps_of
                ctx = env.ctx
                shape = (65, 129)            # of test_gpu_flow_smooth.SHAPES: one past the 64 x 128 tile either way
                f, rng = make_flow(*shape)
                weight, cells = make_weight(kind, *shape, rng)
                taps = taps_of(r)
                exp = {mode: R.smooth_flow_ref(f, taps, weight, cells, mode, 1e-3) for mode in ("all", "blend")}

                def run():
                    d, dw = dev(ctx, f, weight)
                    got = {}
                    for mode in ("all", "blend"):
                        out, info = ctx.smooth_flow(d, taps, dw, cells, mode, 1e-3, return_info=True)
                        into = ctx.smooth_flow(d, taps, dw, cells, mode, 1e-3, out=ctx.empty(shape + (2,), F32))
                        assert_same(into.numpy(), out.numpy(), "into a poisoned out")
                        got[mode] = (out.numpy(), info.unsupported)
                    return got
                return run, exp
        _smooth()


@case("fold_mask", "ma_flow_fold_mask")
def _(env):
    import _flow_smooth_ref as R
    from test_gpu_flow_smooth import folding_flow, odd_values
    ctx = env.ctx
    f = odd_values(folding_flow(*SHAPE), None)
    exp = [R.fold_mask_ref(f, margin) for margin in (0, 2, 32)]

    def run():
        got = []
        for margin in (0, 2, 32):
            keep, info = ctx.fold_mask(dev(ctx, f), margin, return_info=True)
            got.append((keep.numpy(), tuple(info)))
        return got
    return run, exp


for _kind in KINDS:
    def _median(kind=_kind):
        @case(f"median_flow[{kind}]", "ma_median_flow")
        def _(env):
            import _flow_median_ref as R
            from test_gpu_flow_median import make_flow, make_weight
            ctx = env.ctx
            shape = (40, 257)                # of test_gpu_flow_median.SHAPES: past the 32 x 64 tile either way
            f, rng = make_flow(*shape)
            weight, cells = make_weight(kind, *shape, rng)
            plan = [(2, "outliers", 0.5, False), (2, "all", np.inf, True), (4, "all", 0.5, False)]   # register, generic, r > 3
            exp = []
            for r, mode, thresh, generic in plan:
                m, part, n = R.window_median(f, r, weight, cells)
                exp.append(tuple(R.finish(f, m, part, n, mode, thresh)))

            def run():
                d, dw = dev(ctx, f, weight)
                got = []
                for r, mode, thresh, generic in plan:
                    out, keep, info = ctx.median_flow(d, r, dw, cells, mode, thresh, return_info=True, keep=True, generic=generic)
                    into = ctx.median_flow(d, r, dw, cells, mode, thresh, out=ctx.empty(shape + (2,), F32), generic=generic)
                    assert_same(into.numpy(), out.numpy(), "into a poisoned out")
                    got.append((out.numpy(), keep.numpy(), tuple(info)))
                return got
            return run, exp

        @case(f"fill_flow[{kind}]", "ma_fill_flow")
        def _(env):
            import _flow_fill_ref as R
            from test_gpu_flow_fill import make_flow, make_weight
            ctx = env.ctx
            shape = (65, 129)                # of test_gpu_flow_fill.SHAPES
            f, rng = make_flow(*shape)
            f[rng.random(shape) < 0.02] = np.nan
            weight, cells = make_weight(kind, *shape, rng)
            e, counts, levels = R.fill_flow_ref(f, weight, cells)
            exp = (e, tuple(counts) + (levels,))

            def run():
                d, dw = dev(ctx, f, weight)
                out, info = ctx.fill_flow(d, dw, cells, return_info=True)
                into = ctx.fill_flow(d, dw, cells, out=ctx.empty(shape + (2,), F32))
                assert_same(into.numpy(), out.numpy(), "into a poisoned out")
                return out.numpy(), tuple(info)
            return run, exp
    _median()


@case("texture_maps", "ma_texture_maps")
def _(env):
    import _texture_ref as T
    from test_gpu_flow_smooth import taps_of
    from test_gpu_texture import CELLS, floor_of, make_image
    ctx = env.ctx
    planes = ("lam_min", "lam_max", "weight")
    cases = []
    for r, dtype in ((7, np.uint16), (128, np.uint8), (2, np.float32)):
        img, taps = make_image(65, 129, dtype), taps_of(r)          # (65, 129): of test_gpu_flow_smooth.SHAPES
        floor = floor_of(T.texture_maps_ref(img, taps))
        cases.append((img, taps, floor))
    exp = []
    for img, taps, floor in cases:
        ref = T.texture_maps_ref(img, taps, floor, CELLS)
        exp.append(dict({n: ref[n] for n in planes}, counts=ref["counts"]))

    def run():
        got = []
        for img, taps, floor in cases:
            g = ctx.texture_maps(dev(ctx, img), taps, floor, CELLS, planes)
            got.append(dict({n: g[n].numpy() for n in planes}, counts=g["counts"]))
        return got
    return run, exp


@case("local_correlation", "ma_local_correlation")
def _(env):
    import _local_correlation_ref as R
    from test_gpu_flow_smooth import taps_of
    from test_gpu_local_correlation import CELLS, PLANES, centres, make_pair, make_weight
    ctx = env.ctx
    shape = (65, 129)
    w, mask = make_weight(*shape)
    cases = []
    for r, dtype, weight, kw in ((7, np.uint16, None, {}), (49, np.uint8, w, dict(min_support=0.3, lo=-0.5, hi=0.9)),
                                 (2, np.float32, mask, dict(min_support=0.05))):
        ref, img, floor = make_pair(*shape, dtype)
        cases.append((ref, img, taps_of(r), floor, centres(ref, img), weight, kw))
    exp = []
    for ref, img, taps, floor, c, weight, kw in cases:
        e = R.local_correlation_ref(ref, img, taps, floor, c, weight, cell_size=CELLS, **kw)
        exp.append(dict({n: e[n] for n in PLANES}, counts=e["counts"]))

    def run():
        got = []
        for ref, img, taps, floor, c, weight, kw in cases:
            g = ctx.local_correlation(*dev(ctx, ref, img), taps, floor, c, dev(ctx, weight), cell_size=CELLS, want=PLANES, **kw)
            got.append(dict({n: g[n].numpy() for n in PLANES}, counts=g["counts"]))
        return got
    return run, exp


@case("flow_refine_step", "ma_flow_refine_step")
def _(env):
    import _flow_refine_ref as R
    from test_gpu_flow_refine import floor_of, make_case, taps_of
    ctx = env.ctx
    shape = (65, 129)                        # of test_gpu_flow_refine.SHAPES
    rng = np.random.default_rng(4)
    wf = rng.uniform(0.1, 2, shape).astype(F32)
    wf[rng.random(shape) < 0.2] = 0
    wu = (rng.random(shape) < 0.6).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    cases = [make_case(*shape, dt) + (taps_of(r), floor_of(dt), wt)
             for r, dt, wt in ((12, np.uint8, None), (1, np.uint16, wf), (128, np.float32, wu))]
    exp = []
    for ref, wp, flow, taps, floor, wt in cases:
        e, s = R.step(ref, wp, flow, taps, floor, wt, 1.0)
        exp.append((e, (float(s.step_max), int(s.clamped), int(s.invalid))))

    def run():
        got = []
        for ref, wp, flow, taps, floor, wt in cases:
            d = dev(ctx, ref, wp, flow)
            out, info = ctx.flow_refine_step(*d, taps, floor, dev(ctx, wt), 1.0, return_info=True)
            into = ctx.flow_refine_step(*d, taps, floor, dev(ctx, wt), 1.0, out=ctx.empty(shape + (2,), F32))
            assert_same(into.numpy(), out.numpy(), "into a poisoned out")
            got.append((out.numpy(), (float(info.step_max), int(info.clamped), int(info.invalid))))
        return got
    return run, exp


U = 2.0 ** -53


@case("flow_affine_moments, flow_affine_apply", ("ma_flow_affine_moments", "ma_flow_affine_apply"))
def _(env):
    import _flow_affine_ref as R
    from test_gpu_flow_affine import make_flow, make_weight
    ctx = env.ctx
    H, W = 65, 511                           # of test_gpu_flow_affine.SHAPES: one row and one column past the 64 x 510 tile
    f, rng = make_flow(H, W, odd=True)
    near = np.array([[1.02, 0.003, -0.4], [-0.002, 0.99, 0.3]])
    plan = [("none", None, None, None), ("f32", (32, 50), None, None), ("u8", None, near, 1.5), ("cells", (32, 50), near, 1.5)]
    plan = [(make_weight(kind, H, W, np.random.default_rng(7), cells), cells, prior, clip) for kind, cells, prior, clip in plan]
    exp = [R.moments_ref(f, weight, cells, prior, clip) for weight, cells, prior, clip in plan]
    A = np.array([[0.99, 0.02, 1.5], [-0.015, 1.01, -2.25]])
    applied = R.apply_ref(f, A)

    def run():
        d = dev(ctx, f)
        got = [ctx.flow_affine_moments(d, dev(ctx, weight), cells, prior, clip) for weight, cells, prior, clip in plan]
        out = ctx.flow_affine_apply(d, A)
        into = ctx.flow_affine_apply(d, A, out=ctx.empty((H, W, 2), F32))
        assert_same(into.numpy(), out.numpy(), "into a poisoned out")
        return got, out.numpy()

    def check(got):
        # check_moments of tests/test_gpu_flow_affine.py: counts equal, every sum within (n + 1) 2^-53 sum |term| of the fsum
        moments, out = got
        for (sums, counts), (e, ecounts, eabs) in zip(moments, exp):
            assert np.array_equal(counts, ecounts)
            assert np.all(np.abs(sums - e) <= (ecounts[..., :1] + 1) * U * eabs)
            assert np.all(sums[ecounts[..., 0] == 0] == 0.0)
        assert_same(out, applied, "flow_affine_apply")
    return run, check


@case("direct_affine_moments, mask_weight", ("ma_direct_affine_moments", "ma_direct_mask_weight"))
def _(env):
    import _direct_affine_ref as R
    from test_gpu_direct_affine import images, make_weight
    ctx = env.ctx
    plan = []
    for shape, rd, md, kind, clip in (((96, 161), np.uint16, np.float32, "f32", None), ((37, 515), np.uint8, np.uint16, "u8", 20.0),
                                      ((96, 161), np.float32, np.uint8, "none", None)):
        ref, mov, M = images(shape, rd, md)
        plan.append((ref, mov, M, 0.9, 2.0, make_weight(kind, shape), clip))
    exp = [R.moments_ref(*p) for p in plan]
    mask = plan[1][5]

    def run():
        got = [ctx.direct_affine_moments(*dev(ctx, ref, mov), M, gain, bias, dev(ctx, weight), clip)
               for ref, mov, M, gain, bias, weight, clip in plan]
        return got, ctx.mask_weight(dev(ctx, mask)).numpy()

    def check(got):
        # check_moments of tests/test_gpu_direct_affine.py
        moments, w = got
        for (sums, counts), (e, ecounts, eabs) in zip(moments, exp):
            assert np.array_equal(counts, ecounts), (counts, ecounts)
            assert np.all(np.abs(sums - e) <= (ecounts[0] + 1) * U * eabs)
        assert_same(w, (mask != 0).astype(F32), "mask_weight")
    return run, check


@case("landmark_flow, landmark_points", ("ma_landmark_flow", "ma_landmark_points"))
def _(env):
    import _landmarks_ref as R
    from test_gpu_landmarks import statement_flow, synthetic
    ctx = env.ctx
    H, W, n = 37, 515, 130                   # of test_gpu_landmarks.SHAPES: three blocks of 256 columns, the last ragged
    cw, a6, c, k, r = synthetic(H, W, n, "integer")
    flows = [statement_flow(H, W, n, "integer", stride) for stride in (1, 8)]
    rng = np.random.default_rng(n + 7)
    p = np.concatenate([r, rng.random((400, 2)) * [W - 1, H - 1], (rng.random((150, 2)) - 0.5) * [8 * W, 8 * H]])
    pexp, mag = R.evaluate(cw, a6, c, k, p)

    def run():
        return [ctx.landmark_flow(cw, a6, c, k, (H, W), stride).numpy() for stride in (1, 8)], ctx.landmark_points(cw, a6, c, k, p)

    def check(got):
        # the derived bounds of tests/test_gpu_landmarks.py: check_flow and the points test
        for g, (e, bound) in zip(got[0], flows):
            assert g.dtype == F32 and g.shape == e.shape and np.all(np.isfinite(g))
            assert np.all(np.abs(g.astype(F64) - e) <= bound + 2.0 ** -23 * np.maximum(1.0, np.abs(e)))
        assert got[1].dtype == F64 and got[1].shape == p.shape and np.all(np.isfinite(got[1]))
        assert np.all(np.abs(got[1] - pexp) <= R.bound(mag, n))
    return run, check
