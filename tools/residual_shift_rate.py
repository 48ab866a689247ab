"""Rate of the residual shift maps on a device-resident 16384^2 pair of u8 label images.

    python tools/residual_shift_rate.py [size] [--cell N] [--reps K] [--shifts 4 8]

Times ma_residual_shift_grid (the reference against two label images, as residual_shift() calls it) end to end (wall clock,
inputs already in HBM) and its correlation kernel alone through the library's per-kernel accounting (ma_profile_*, HIP
events around the launch), for every max_shift asked for: the median of `reps` calls after a warm-up, with the minimum and
the maximum.  The histogram pass of the registration quality maps (ma_qc_nmi_grid on the same three images) is timed the
same way as the yardstick.  Rates are dot4 lane-operations of the S_ab sums (pixels x shifts x images / 4) per second."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=16384)
    ap.add_argument("--cell", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shifts", type=int, nargs="+", default=[4, 8])
    a = ap.parse_args()
    H = W = a.size
    rng = np.random.default_rng(0)
    ref = rng.integers(0, 256, (H, W), dtype=np.uint8)
    after = np.roll(ref, (0, 1), axis=(0, 1))
    after[::5] = rng.integers(0, 256, after[::5].shape, dtype=np.uint8)
    before = np.roll(ref, (3, -2), axis=(0, 1))
    ctx = get_context()
    d_ref, d_after, d_before = ctx.asdevice(ref), ctx.asdevice(after), ctx.asdevice(before)
    del ref, after, before
    ctx.sync()
    ctx.profile(True)
    try:
        for R in a.shifts:
            res = {}

            def call():
                res["m"] = ctx.residual_shift_grid(d_ref, d_after, d_before, a.cell, a.cell, R)
            walls, kern = timed(ctx, call, a.reps)
            m0, m1 = res["m"]
            ops = 2.0 * (H - 2 * R) * (W - 2 * R) * (2 * R + 1) ** 2 / 4
            print(f"ma_residual_shift_grid {H}x{W} u8, cells of {a.cell} ({m0['valid'].size}), max_shift {R}, 2 label images: "
                  f"wall {fmt(walls)}; correlation kernel {fmt(kern)} = {ops / np.median(kern) / 1e9:.1f} T dot4 lane-ops/s; "
                  f"median |shift| after {np.median(np.hypot(m0['shift_x'], m0['shift_y'])):.3f}, "
                  f"before {np.median(np.hypot(m1['shift_x'], m1['shift_y'])):.3f} px, at the limit {int(m1['at_limit'].sum())}")
        walls, kern = timed(ctx, lambda: ctx.qc_nmi_grid(d_ref, d_after, d_before, a.cell, a.cell), a.reps)
        print(f"yardstick ma_qc_nmi_grid, the same images: wall {fmt(walls)}; histogram pass {fmt(kern)}")
    finally:
        ctx.profile(False)


if __name__ == "__main__":
    main()
