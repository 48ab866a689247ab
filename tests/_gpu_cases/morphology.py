"""Cases of the registry: the flat grey morphology."""
import numpy as np

from .registry import SHAPE, case, dev


def _case(name, dtype, op, radius, in_place):
    @case(name, "ma_morphology")
    def make(env):
        import _morph_ref as R
        ctx = env.ctx
        img = R.make_image(*SHAPE, dtype, 11)
        exp = R.morphology_ref(img, op, radius)

        def run():
            d_img = dev(ctx, img)
            if in_place:
                work = d_img.copy()       # the uploaded array stays what the host array holds
                out = ctx.morphology(work, op, radius, out=work)
                assert out is work
            else:
                out = ctx.morphology(d_img, op, radius)
            return out.numpy()
        return run, exp
    return make


# a radius above one block of halo on both axes, with block minima (r >= 16) and without (8 <= r < 16)
_case("morphology[uint16, tophat, r=(21, 40)]", np.uint16, "tophat", (21, 40), False)
_case("morphology[float32, close in place, NaNs, r=(9, 3)]", np.float32, "close", (9, 3), True)
_case("morphology[uint8, erode, r=(2, 255)]", np.uint8, "erode", (2, 255), False)
