"""Cases of the registry: DOG."""
import ctypes as C

import numpy as np

from .registry import F32, SHAPE, _O, case, dev, pair


_DT = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}


@case("dog_u8[every entry, every flag, every sigma pair of the suite]", ("ma_dog_u8", "ma_dog_u8_minmax", "ma_dog_u8_ex"))
def _(env):
    O = _O()
    ctx = env.ctx
    h, w = SHAPE
    imgs = [pair(h, w, seed=301, dtype=dt)[0] for dt in (np.uint8, np.uint16, np.float32)]
    sigmas = [(5, 9), (1, 2), (3, 5), (6, 9)]
    flags = [0, O.DOG_FUSED_BLUR, O.DOG_FUSED_SCALE, O.DOG_FUSED]
    exp = {}
    for k, img in enumerate(imgs):
        for s in sigmas:
            for fl in flags:
                exp[k, s, fl] = O.dog(img, True, *s, flags=fl)
        exp[k, "plain"] = (exp[k, (5, 9), 0], 0)
        exp[k, "minmax"] = (exp[k, (5, 9), 0], 0)
    exp["zero"] = (np.zeros((h, w), np.uint8), True)

    def run():
        got = {}
        for k, img in enumerate(imgs):
            d = dev(ctx, img)
            for s in sigmas:
                for fl in flags:
                    got[k, s, fl] = ctx.dog_u8(d, *s, flags=fl).numpy()
            flag = C.c_int(-1)
            out = ctx.empty((h, w), np.uint8)
            ctx._run(ctx.lib.ma_dog_u8, d.ptr, _DT[d.dtype], h, w, 5, 9, out.ptr, C.byref(flag))
            got[k, "plain"] = (out.numpy(), flag.value)
            mm = dev(ctx, np.array([img.min(), img.max()], F32))
            flag = C.c_int(-1)
            out = ctx.empty((h, w), np.uint8)
            ctx._run(ctx.lib.ma_dog_u8_minmax, d.ptr, _DT[d.dtype], h, w, 5, 9, mm.ptr, out.ptr, C.byref(flag))
            got[k, "minmax"] = (out.numpy(), flag.value)
        out, zero = ctx.dog_u8(dev(ctx, np.zeros((h, w), F32)), report_zero=True)
        got["zero"] = (out.numpy(), zero)
        return got
    return run, exp
