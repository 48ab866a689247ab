"""Cases of the registry: the whole path."""
from .registry import _RO, assert_same, case, dev, pair


REGISTER = dict(num_pyr_lvl=2, tile_size=100, overlap=20, use_dog=True)

for _on in (True, False):
    def _register(on=_on):
        @case(f"optflow_register[companion stream {'on' if on else 'off'}]", "ma_optflow_register")
        def _(env):
            ctx = env.ctx
            ref, mov = pair(420, 404, seed=21)
            flow, reports = _RO().register(ref, mov, **REGISTER)
            exp = (flow, [r[3] for r in reports])

            def run():
                ctx.companion_stream = on
                try:
                    f, reps = ctx.optflow_register(*dev(ctx, ref, mov), **REGISTER)
                    return f.numpy(), [r[4] for r in reps], [r[:4] for r in reps]
                finally:
                    ctx.companion_stream = True

            def check(got):
                # test_register_matches_oracle_orchestration: the flow bit for bit, the same levels accepted
                assert_same(got[:2], exp, "register")
            return run, check
    _register()
