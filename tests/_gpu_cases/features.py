"""Cases of the registry: features."""
import numpy as np

from .registry import F32, _O, assert_same, case, dev


def _tables():
    from microaligner_amd.feature_reg import feature_detection as FD
    from microaligner_amd.feature_reg.sparse_cpu import Daisy
    return FD._daisy_tables(Daisy(radius=21, q_radius=3, q_theta=8, q_hist=8))


@case("cut_tiles, fast_nms, fast_keypoints", ("ma_cut_tiles_u8", "ma_fast_nms", "ma_fast_keypoints"))
def _(env):
    import test_feature_edges_ref as R
    ctx = env.ctx
    img, feat = R.dense_case()               # 4 x 4 windows with ragged remainders
    tile, nms = R.nms_case(257, 3)           # one past a block of 256 threads
    tiles, maps = R.multi_tiles()            # an all-zero tile, a constant one, two corners, 8464 equal ones, 8193 mixed
    stack = np.ascontiguousarray(np.stack(tiles))
    limit = 100

    def run():
        counts, kp = ctx.fast_keypoints(dev(ctx, stack), 3, limit)
        # rows beyond counts[t] are undefined: what is compared is what selection_mismatch compares
        return (ctx.cut_tiles(dev(ctx, img), R.TILE, R.OV, 0, len(feat.windows)).numpy(),
                ctx.fast_nms(dev(ctx, np.ascontiguousarray(tile[None])), 3), counts,
                [kp[t, :counts[t]].copy() for t in range(len(tiles))])

    def check(got):
        windows, score, counts, kps = got
        assert np.array_equal(windows, np.stack(feat.windows))
        assert score.shape == (1, 257, 257) and np.array_equal(score[0], nms)
        for t in range(len(tiles)):
            bad = R.selection_mismatch(counts[t], kps[t], R.expected_selection(maps[t], limit), int((maps[t] > 0).sum()), limit)
            assert bad is None, (t, bad)
    return run, check


@case("daisy_describe", "ma_daisy_describe")
def _(env):
    import test_feature_edges_ref as R
    ctx = env.ctx
    windows, pts, desc = [], [], []
    for shape in ((40, 61), (63, 4)):
        img, feat = R.single_case(shape)
        windows.append(feat.windows[0])
        pts.append(feat.pts)
        desc.append(feat.desc)
    stack = np.ascontiguousarray(np.stack(windows))
    kp_tile = np.concatenate([np.full(len(p), t, np.int32) for t, p in enumerate(pts)])
    kp_xy = np.concatenate(pts)
    return (lambda: ctx.daisy_describe(dev(ctx, stack), kp_tile, kp_xy, *_tables())), np.concatenate(desc)


@case("feature_extract[waited, enqueued, in batches]", ("ma_feature_extract", "ma_feature_extract_enqueue"))
def _(env):
    import test_feature_edges_ref as R
    from test_gpu_feature_edges import _extract
    ctx = env.ctx
    img, feat = R.dense_case()
    rimg, rfeat = R.remainder_case((251, 299))
    P = R.TILE + 2 * R.OV

    def run():
        d, dr = dev(ctx, img, rimg)
        return ([_extract(ctx, d, 12, workspace_bytes=k * 128 * P * P, wait=wait) for k in (0, 2) for wait in (True, False)],
                _extract(ctx, dr, 12))

    def check(got):
        for g in got[0]:
            bad = R.features_mismatch(g, feat)
            assert bad is None, bad
        bad = R.features_mismatch(got[1], rfeat)
        assert bad is None, bad
    return run, check


def _knn(kind, nq, nt, dim):
    @case(f"knn2[{kind},{nq}x{nt}x{dim}]", ("ma_knn2_l2_ex", "ma_knn2_l2"))
    def _(env):
        from microaligner_amd.feature_reg import sparse_cpu as SP
        from test_feature_reg import _knn_case
        ctx = env.ctx
        q, t = _knn_case(kind, nq, nt, dim, seed=nq + nt)
        exp = SP.knn2_sequential(q, t) if nq * nt <= 3000 * 5000 else None

        def run():
            dq, dt = dev(ctx, q, t)
            got = {}
            for mode in ("exact", "filtered", "filtered_f32", "auto"):
                stats = {}
                got[mode] = ctx.knn2(dq, dt, mode=mode, stats=stats) + (stats["uncertified"],)
            idx, dist = ctx.empty((nq, 2), F32), ctx.empty((nq, 2), F32)
            ctx._run(ctx.lib.ma_knn2_l2, dq.ptr, nq, dt.ptr, nt, dim, idx.ptr, dist.ptr)
            got["ma_knn2_l2"] = (idx.numpy().view(np.int32).astype(np.int64), np.sqrt(dist.numpy()))
            return got

        def check(got):
            # test_filtered_knn2_equals_the_exact_search: every mode gives the exact kernel's bits, and those are the float32
            # definition's where that is quick enough to state
            for mode, g in got.items():
                assert_same(g[:2], got["exact"][:2], mode)
            if exp is not None:
                assert_same(got["exact"][:2], exp, "the float32 definition")
        return run, check


for _args in [("uniform", 1000, 3000, 200), ("uniform", 129, 1000, 200), ("uniform", 1, 2, 200), ("uniform", 300, 5, 8),
              ("uniform", 257, 131, 216), ("uniform", 64, 700, 12), ("histograms", 2500, 4100, 200), ("duplicates", 500, 1500, 200),
              ("near_ties", 200, 900, 200), ("uniform", 6000, 9000, 200), ("wide_range", 700, 2100, 200), ("tiny", 400, 1300, 200),
              ("outlier", 500, 1500, 200), ("clusters", 900, 2600, 200), ("histograms", 333, 1111, 44), ("uniform", 200, 600, 208)]:
    _knn(*_args)


@case("match_similarity", "ma_match_similarity")
def _(env):
    import test_match_ref as R
    from test_gpu_match import _call
    ctx = env.ctx
    names = ("second_instalment", "n_good_1", "large_refused_n64", "max_iters_1", "nq_3100_noisy", "nq_65_noisy")
    exp = [tuple(R.expected(R.BY_NAME[n])[:3]) for n in names]
    return (lambda: [_call(ctx, R.BY_NAME[n]) for n in names]), exp


def _round_images(dtype):
    from microaligner_amd import synthetic
    O = _O()
    H, W = 420, 404
    ref = synthetic.make_cells(H, W, seed=33, dtype=dtype)
    th = np.deg2rad(-0.5)
    mov = O.warp_affine(ref, np.array([[np.cos(th), -np.sin(th), -8.0], [np.sin(th), np.cos(th), 5.0]]))
    return ref, mov


for _use_dog, _dtype in ((True, np.uint16), (False, np.uint8)):
    def _round(use_dog=_use_dog, dtype=_dtype):
        @case(f"feature_round[use_dog={use_dog},{np.dtype(dtype).name}]", "ma_feature_round")
        def _(env):
            from microaligner_amd.feature_reg import feature_detection as FD
            ctx = env.ctx
            tile, chunk = 200, 200 * 200
            ref, mov = _round_images(dtype)
            tables = _tables()

            def step_by_step():
                """the calls ma_feature_round chains, one by one (test_fused_round_equals_the_step_by_step_entry_points)"""
                dref, dmov = dev(ctx, ref, mov)
                ref_gate, gate = ctx.dog_u8(dref), ctx.dog_u8(dmov)
                fr = FD.find_features_of_device_image(ref_gate if use_dog else dref, tile, ctx)
                fm = FD.find_features_of_device_image(gate if use_dog else dmov, tile, ctx)
                idx, dist = ctx.knn2(fm.descriptors_for_search, fr.descriptors_for_search, on_device=True)
                mat, n_good, status = ctx.match_similarity(idx, dist, fm.device_pts(ctx), fr.device_pts(ctx),
                                                           n_train=len(fr.descriptors_for_search))
                assert status == 0 and n_good > 20, (status, n_good)
                cand = ctx.warp_affine_cv(dmov, mat)
                cand_gate = ctx.dog_u8(cand)
                after, before = ctx.nmi_scores_pair(ref_gate, cand_gate, gate, chunk)
                return dict(estimate=mat, n_query=len(fm.descriptors_for_search), n_good=n_good, status=status, after=after,
                            before=before, gate=gate.numpy(), candidate=cand.numpy(), candidate_gate=cand_gate.numpy())
            exp = step_by_step()

            def run():
                dref, dmov = dev(ctx, ref, mov)
                ref_gate = ctx.dog_u8(dref)
                fr = FD.find_features_of_device_image(ref_gate if use_dog else dref, tile, ctx)
                feats = (fr.descriptors_for_search, fr._dev[1], fr._dev[3])
                r = ctx.feature_round(dmov, None, ref_gate, feats, tile, use_dog, chunk, *tables)
                assert not r["zero_max"] and not r["is_identity"]
                return dict(estimate=r["estimate"], n_query=r["n_query"], n_good=r["n_good"], status=r["status"],
                            after=r["scores_after"], before=r["scores_before"], gate=r["current_gate"].numpy(),
                            candidate=r["candidate"].numpy(), candidate_gate=r["candidate_gate"].numpy())
            return run, exp
    _round()
