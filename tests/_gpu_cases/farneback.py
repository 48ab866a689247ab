"""Cases of the registry: Farneback."""
import numpy as np

from .registry import _O, _RO, case, dev, pair


def _farneback(name, shape, win, iters, seed, oracle, **kw):
    @case(name, "ma_farneback_tiled")
    def make(env):
        ctx = env.ctx
        ref, mov = pair(*shape, seed=seed)
        exp = oracle(ref, mov)
        return (lambda: ctx.farneback(*dev(ctx, mov, ref), win, iters, **kw).numpy()), exp


_farneback("farneback[untiled]", (131, 157), 19, 3, 150, lambda ref, mov: _O().calc_optical_flow_farneback(mov, ref, 19, 3))
_farneback("farneback[fused]", (140, 150), 31, 3, 8,
           lambda ref, mov: _O().calc_optical_flow_farneback(mov, ref, 31, 3, fused=True), fused=True)
# ragged right and bottom windows that are mostly padding: what the active-extent and needed-rectangle arguments are about
_farneback("farneback[tiled]", (250, 310), 19, 3, 100, lambda ref, mov: _RO().tile_flow(ref, mov, 100, 20, 19, 3),
           tile=100, overlap=20)
_farneback("farneback[tiled,fused]", (250, 310), 19, 3, 100,
           lambda ref, mov: _RO().tile_flow(ref, mov, 100, 20, 19, 3, fused=True), tile=100, overlap=20, fused=True)
_farneback("farneback[fallback kernels]", (40, 700), 601, 2, 5,
           lambda ref, mov: _O().calc_optical_flow_farneback(mov, ref, 601, 2))


@case("farneback[tiled,batches under an 8 MiB workspace]", "ma_farneback_tiled")
def _(env):
    from microaligner_amd import _lib as L
    ctx = env.ctx
    ref, mov = pair(250, 310, seed=100)
    exp = _RO().tile_flow(ref, mov, 100, 20, 19, 3)

    def run():
        # one 140 x 140 window takes 140 * 192 * 4 * 20 B = 2.05 MiB of planes: 8 MiB forces batches of 3 windows
        L.check(ctx.lib.ma_ctx_set_workspace_limit(ctx.handle, 8 << 20))
        try:
            return ctx.farneback(*dev(ctx, mov, ref), 19, 3, tile=100, overlap=20).numpy()
        finally:
            L.check(ctx.lib.ma_ctx_set_workspace_limit(ctx.handle, 48 << 30))
    return run, exp


@case("farneback[levels=2]", "ma_farneback_levels")
def _(env):
    from test_gpu_farneback_levels import _pair
    ctx = env.ctx
    mov, ref = _pair(131, 157, np.float32)
    exp = env.levels.farneback(mov, ref, 2, 15, 3, fused=False)
    return (lambda: ctx.farneback(*dev(ctx, mov, ref), 15, 3, levels=2).numpy()), exp


@case("farneback_debug", "ma_farneback_debug")
def _(env):
    ctx = env.ctx
    ref, mov = pair(150, 170, 3)
    flow, r0, r1, m0 = _O().calc_optical_flow_farneback(mov, ref, 21, 1, dump=True)
    exp = (flow,) + tuple(np.ascontiguousarray(np.moveaxis(a, 2, 0)) for a in (r0, r1, m0))
    return (lambda: tuple(a.numpy() for a in ctx.farneback_debug(*dev(ctx, mov, ref), 21, 1))), exp
