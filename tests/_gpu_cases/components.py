"""Cases of the registry: the connected components."""
import numpy as np

from .registry import SHAPE, case


@case("components[uint8, label with info, 8 neighbours]", ("ma_cc_label", "ma_cc_stats"))
def _label(env):
    import _components_ref as R
    ctx = env.ctx
    img = R.random_mask(*SHAPE, 0.45, 41) * np.uint8(200)
    labels, n = R.label_ref(img, 2)
    exp = (labels, n) + R.stats_ref(labels, n)

    def run():
        d_labels, count = ctx.label_components(ctx.components_asdevice(img), 2)
        areas, bboxes = ctx.component_stats(d_labels, count)
        return d_labels.numpy(), count, areas.numpy(), bboxes.numpy()
    return run, exp


@case("components[uint16, objects by value in place, an odd element offset]", "ma_cc_filter")
def _objects(env):
    import _components_ref as R
    ctx = env.ctx
    img = np.random.default_rng(42).integers(0, 3, SHAPE).astype(np.uint16) * np.uint16(30000)
    exp = R.remove_small_ref(img, 6, 1, True)
    assert 0 < np.count_nonzero(exp) < np.count_nonzero(img)

    def run():
        work = ctx.components_asdevice(img).copy()       # the uploaded array stays what the host array holds
        out = ctx.remove_small_objects(work, 6, 1, True, out=work)
        assert out is work
        return out.numpy()
    return run, exp


@case("components[int32, holes up to a size]", "ma_cc_filter")
def _holes(env):
    import _components_ref as R
    ctx = env.ctx
    img = R.random_mask(*SHAPE, 0.62, 43).astype(np.int32) * np.int32(-7)
    exp = R.fill_holes_ref(img, 9, 1, 2 ** 31 - 1)
    full = R.fill_holes_ref(img, None, 1, 2 ** 31 - 1)
    assert 0 < np.count_nonzero(exp != img) < np.count_nonzero(full != img)

    def run():
        return ctx.fill_holes(ctx.components_asdevice(img), 9, 1, 2 ** 31 - 1).numpy()
    return run, exp
