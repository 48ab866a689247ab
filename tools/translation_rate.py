"""Rate of the global translation search (include/microaligner_translation.h) on device-resident u8 label images.

    python tools/translation_rate.py [--size N] [--coarse N] [--reps K] [--no-whole]

Times, as the median of `reps` calls after a warm-up, with the minimum and the maximum:
 - the coarse search: ma_translation_search of a `coarse`^2 pair (512) over +-coarse/2 per axis, end to end (wall clock, labels
   already in HBM) and its correlation kernel alone through the library's per-kernel accounting (HIP events around the launch);
 - a level-0 refinement: ma_translation_search of a `size`^2 pair (16384) over 25 shifts off the centre, the same two figures;
 - a whole align_translation of a `size`^2 uint8 pair with the default coarse_side, "u8" labels, inputs in HBM;
 - the yardstick: ma_residual_shift_grid of the `size`^2 pair at max_shift 8, cells of 1000, one label image.
Rates are dot4 lane-operations of the S_ab sums (pixels of the overlap x shifts / 4) per second."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from microaligner_amd import align_translation
from microaligner_amd.device import get_context


def timed(ctx, fn, reps):
    """(wall ms, profiled ms of the 'other' kernels) of `reps` calls after one warm-up call."""
    fn()
    walls, kern = [], []
    for _ in range(reps):
        ctx.profile_reset()
        t0 = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t0) * 1e3)
        kern.append(ctx.profile_get()["other"]["ms"])
    return walls, kern


def fmt(v):
    return f"{np.median(v):.3f} ms median (min {min(v):.3f}, max {max(v):.3f})"


def overlap_ops(h, w, window):
    dx0, dx1, dy0, dy1 = window
    return sum(max(0, h - abs(dy)) for dy in range(dy0, dy1 + 1)) * sum(max(0, w - abs(dx)) for dx in range(dx0, dx1 + 1)) / 4.0


def shifted_pair(n, shift, seed):
    """u8 noise, smoothed a little so that a pyramid keeps it, and the same moved by `shift`: a(p) = b(p + shift)"""
    rng = np.random.default_rng(seed)
    m = max(abs(shift[0]), abs(shift[1]))
    big = rng.integers(0, 256, (n + 2 * m, n + 2 * m), dtype=np.uint8)
    big = ((big.astype(np.uint16) + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) // 4).astype(np.uint8)
    a = np.ascontiguousarray(big[m:m + n, m:m + n])
    b = np.ascontiguousarray(big[m - shift[1]:m - shift[1] + n, m - shift[0]:m - shift[0] + n])
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--coarse", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-whole", action="store_true")
    a = ap.parse_args()
    ctx = get_context()
    shift = (301, -212)
    ref, mov = shifted_pair(a.size, shift, 0)
    d_ref, d_mov = ctx.asdevice(ref), ctx.asdevice(mov)
    c_ref, c_mov = (ctx.asdevice(x) for x in shifted_pair(a.coarse, (shift[0] * a.coarse // a.size, shift[1] * a.coarse // a.size), 1))
    del ref, mov
    ctx.sync()
    ctx.profile(True)
    try:
        r = a.coarse // 2
        for name, x, y, n, window in (("coarse search", c_ref, c_mov, a.coarse, (-r, r, -r, r)),
                                      ("level-0 refinement", d_ref, d_mov, a.size,
                                       (shift[0] - 2, shift[0] + 2, shift[1] - 2, shift[1] + 2))):
            res = {}

            def call():
                res["r"] = ctx.translation_search(x, y, window, exclude=2)
            walls, kern = timed(ctx, call, a.reps)
            shifts = (window[1] - window[0] + 1) * (window[3] - window[2] + 1)
            print(f"{name}: ma_translation_search {n}x{n} u8 over {shifts} shifts: wall {fmt(walls)}; correlation kernel {fmt(kern)} = "
                  f"{overlap_ops(n, n, window) / np.median(kern) / 1e9:.2f} T dot4 lane-ops/s; peak ({res['r']['dx']}, {res['r']['dy']}) "
                  f"score {res['r']['score']:.4f}")
        if not a.no_whole:
            res = {}

            def whole():
                res["r"] = align_translation(d_ref, d_mov, labels="u8", return_info=True)
            walls, _ = timed(ctx, whole, a.reps)
            info = res["r"][1]
            print(f"align_translation {a.size}x{a.size} uint8, labels 'u8', coarse_side 512, inputs in HBM: wall {fmt(walls)}; "
                  f"levels {[lv.level for lv in info.levels]}, shift {info.shift}, score {info.score:.4f}, accepted {info.accepted}")
        R = 8
        walls, kern = timed(ctx, lambda: ctx.residual_shift_grid(d_ref, d_mov, None, 1000, 1000, R), a.reps)
        ops = (a.size - 2 * R) ** 2 * (2 * R + 1) ** 2 / 4.0
        print(f"yardstick ma_residual_shift_grid {a.size}x{a.size} u8, cells of 1000, max_shift {R}, one label image: wall {fmt(walls)}; "
              f"correlation kernel {fmt(kern)} = {ops / np.median(kern) / 1e9:.2f} T dot4 lane-ops/s")
    finally:
        ctx.profile(False)


if __name__ == "__main__":
    main()
