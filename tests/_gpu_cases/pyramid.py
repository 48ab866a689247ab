"""Cases of the registry: pyramid, min / max, conversions."""
import numpy as np

from .registry import F32, SHAPE, _O, case, dev


def _image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) * (65535 if dtype == np.uint16 else 255)).astype(dtype)


for _dtype in (np.uint8, np.uint16, np.float32):
    def _pyr(dtype=_dtype):
        tag = np.dtype(dtype).name

        @case(f"pyr_down[{tag}]", "ma_pyr_down")
        def _(env):
            ctx = env.ctx
            img = _image(SHAPE, dtype, 67)
            return (lambda: ctx.pyr_down(dev(ctx, img)).numpy()), _O().pyr_down(img)

        @case(f"pyr_down[{tag},minmax]", "ma_pyr_down_minmax")
        def _(env):
            ctx = env.ctx
            img = _image(SHAPE, dtype, 68)
            exp = _O().pyr_down(img)

            def run():
                p = ctx.pyr_down(dev(ctx, img), minmax=True)
                return p.numpy(), p.minmax.numpy()
            return run, (exp, np.array([exp.min(), exp.max()], F32))

        @case(f"minmax, normalize_minmax_u8, to_f32[{tag}]",
              ("ma_minmax", "ma_normalize_minmax_u8") + (("ma_convert_f32",) if dtype != np.float32 else ()))
        def _(env):
            ctx = env.ctx
            img = _image(SHAPE, dtype, 69)
            exp = ((float(img.min()), float(img.max())), _O().normalize_minmax_u8(img.astype(F32)), img.astype(F32))

            def run():
                d = dev(ctx, img)
                return ctx.minmax(d), ctx.normalize_minmax_u8(d).numpy(), ctx.to_f32(d).numpy()
            return run, exp

        @case(f"image_quantiles, normalize_range_u8[{tag}]", ("ma_image_quantiles", "ma_normalize_range_u8"))
        def _(env):
            import _quantile_ref as Q
            from test_gpu_quantiles import QSETS, image
            ctx = env.ctx
            img = image((301, 517), dtype)          # of test_gpu_quantiles.SHAPES
            img.ravel()[::97] = 0
            sets = [(q, False) for q in QSETS] + [(QSETS[-1], True)]
            lo, hi = (float(v) for v in Q.image_quantiles(img, [0.01, 0.99])[0])
            exp = [Q.image_quantiles(img, q, z) for q, z in sets] + [Q.normalize_range_u8(img, lo, hi)]

            def run():
                d = dev(ctx, img)
                got = []
                for q, z in sets:
                    vals, counts = ctx.image_quantiles(d, q, ignore_zeros=z)
                    got.append((vals, tuple(counts)))
                return got + [ctx.normalize_range_u8(d, lo, hi).numpy()]
            return run, exp
    _pyr()


@case("pyr_up_flow", "ma_pyr_up_flow")
def _(env):
    from test_gpu_primitives import rand_flow
    ctx = env.ctx
    f = rand_flow(40, 50, 11, 5.0)
    exp = [_O().pyr_up(f * F32(s), dstsize=(99, 79)) for s in (1.0, 2.0, 4.0)]
    return (lambda: [ctx.pyr_up_flow(dev(ctx, f), (79, 99), s).numpy() for s in (1.0, 2.0, 4.0)]), exp


@case("max_project", "ma_max_project")
def _(env):
    ctx = env.ctx
    rng = np.random.default_rng(0)
    stack = rng.integers(0, 60000, (5,) + SHAPE).astype(np.uint16)
    fs = (stack / F32(7)).astype(F32)
    fs[1, 0, 0] = np.nan
    fs[2, 30:40, 10:90] = np.nan
    return (lambda: [ctx.max_project(dev(ctx, s)).numpy() for s in (stack, fs)]), [stack.max(0), np.maximum.reduce(fs)]
