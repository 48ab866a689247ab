"""Time of farneback(..., pyr_size=0..4) on device-resident float32 pairs, and what the pyramid's own kernels cost.

    python tools/fb_levels_rate.py [--sizes 4096 5120] [--wins 51 99] [--iters 3] [--reps 3]

Per (size, window, pyr_size): the median over `reps` calls of device-event time around one call (after a warm-up call of
the same shape), the ratio to pyr_size 0, and the library's per-kernel accounting (ma_profile_*) of one call.  For the
level-image kernel (blur + resize of both inputs, MA_K_FB_LEVEL_IMG) it also gives the HBM bytes it must move -- one read
of each input, the row pass written and read back, the level image written -- over its time, against 8 TB/s.
Whole-image Farneback keeps a window's 20 planes (rows padded to 64 floats) within INT32_MAX bytes: 5178^2 is the largest
square image it takes (8192^2 is refused with ValueError, at every pyr_size).
Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from microaligner_amd import farneback, synthetic
from microaligner_amd.device import get_context

PEAK = 8.0e12


def level_img_bytes(H, W, levels, esize=4):
    """bytes the level-image kernels must move for one call: per level k >= 1 and image, the input once, the row pass
    (H x 2 w_k floats) written and read, the (h_k, w_k) image written"""
    total, scale = 0.0, 1.0
    for k in range(1, levels + 1):
        scale *= 0.5
        if W * scale < 32 or H * scale < 32:
            break
        w, h = int(round(W * scale)), int(round(H * scale))
        total += 2 * (esize * H * W + 2 * 4.0 * H * 2 * w + 4.0 * w * h)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 5120])
    ap.add_argument("--wins", type=int, nargs="+", default=[51, 99])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="+", default=[0, 1, 2, 3, 4])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = get_context()
    ea, eb = ctx.event(), ctx.event()
    rows = []
    for n in a.sizes:
        ref, mov = synthetic.make_pair(n, n, seed=2, shift=(24.0, -17.0))
        d_ref, d_mov = ctx.asdevice(ref.astype(np.float32)), ctx.asdevice(mov.astype(np.float32))
        del ref, mov
        ctx.sync()
        for win in a.wins:
            base = None
            for lv in a.levels:
                run = lambda: farneback(d_mov, d_ref, pyr_size=lv, win_size=win, num_iter=a.iters)  # noqa: E731
                run()                                                                             # warm-up
                ctx.sync()
                ms = []
                for _ in range(a.reps):
                    ctx.record(ea)
                    run()
                    ctx.record(eb)
                    ms.append(ctx.elapsed_ms(ea, eb))
                t = float(np.median(ms))
                base = t if lv == 0 else base
                ctx.profile(True)
                try:
                    ctx.profile_reset()
                    run()
                    ctx.sync()
                    prof = {k: round(v["ms"], 3) for k, v in ctx.profile_get().items() if v["launches"]}
                finally:
                    ctx.profile(False)
                row = {"size": n, "win": win, "iters": a.iters, "pyr_size": lv, "ms": round(t, 3),
                       "ratio_to_pyr0": round(t / base, 3) if base else None, "kernels_ms": prof}
                li = prof.get("fb_level_img")
                if li:
                    b = level_img_bytes(n, n, lv)
                    row["level_img_GBps"] = round(b / li / 1e6, 1)
                    row["level_img_share_of_hbm_peak"] = round(b / (li * 1e-3) / PEAK, 3)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        del d_ref, d_mov
    print(json.dumps({"tool": "fb_levels_rate", "results": rows}))


if __name__ == "__main__":
    main()
