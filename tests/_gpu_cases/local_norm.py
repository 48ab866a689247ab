"""Cases of the registry: the local contrast normalisation."""
import numpy as np

from .registry import SHAPE, assert_same, case, dev


def _case(name, dtype, r, kind, want, clip, min_support):
    @case(name, "ma_normalize_local")
    def make(env):
        import _local_norm_ref as R
        from test_gpu_flow_smooth import taps_of
        ctx = env.ctx
        img = R.make_image(*SHAPE, dtype)
        weight = None if kind is None else R.make_weight(*SHAPE)[kind]
        taps, floor = taps_of(r), R.floor_of(dtype)
        e = R.normalize_local_ref(img, taps, floor, clip, weight, min_support)
        exp = ({n: e[n] for n in want}, e["counts"])

        def run():
            d_img, d_w = dev(ctx, img, weight)
            out, info = ctx.normalize_local(d_img, taps, floor, clip, d_w, min_support, want, return_info=True)
            alone = ctx.normalize_local(d_img, taps, floor, clip, d_w, min_support, want[:1])
            assert_same(alone[want[0]].numpy(), out[want[0]].numpy(), "one output alone, without the counts")
            return {n: out[n].numpy() for n in want}, tuple(info)
        return run, exp
    return make


_case("normalize_local[uint16, float weight, both outputs]", np.uint16, 7, 0, ("f32", "u8"), 2.0, 0.3)
_case("normalize_local[uint8, no weight, r=49]", np.uint8, 49, None, ("u8",), 4.0, 0.0)
