"""Rate of one refinement step of a flow (Context.flow_refine_step), include/microaligner_flowrefine.h.

    python tools/flow_refine_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident pair (texture_rate.py's image and a copy shifted by a pixel) and the test
   suite's flow B scaled to 1 px.  Per case the median of `reps` HIP-event timings of one call after a warm-up call, with
   minimum and maximum: one step (in place) at sigma = 4 (r = 12) for a uint8, uint16 and float32 reference, and for the
   float32 one with a uint8 mask, and at r = 128 with and without the mask; Context.warp_affine_flow of the float32 moving
   image, which refine_flow() runs before every step; and Context.texture_maps and Context.smooth_flow(where="all") with the
   same taps on the same box as the yardsticks (the same filter over three planes).
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from flow_smooth_rate import block_mask, device_ms, flow_b, run
from texture_rate import image


def step_kernel(a):
    from microaligner_amd.device import gaussian_taps, get_context
    ctx = get_context()
    n = a.size
    wide = gaussian_taps(128 / 3.0, 127.5 / (128 / 3.0))
    assert len(wide) == 129
    windows = (("sigma 4 (r 12)", gaussian_taps(4.0)), ("r 128         ", wide))
    keep = ctx.asdevice(block_mask(n))
    flow = flow_b(n)
    flow *= np.float32(1 / 25)
    flow = ctx.asdevice(flow)
    identity = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])

    def report(label, fn):
        r = fn()                                        # first launch, the buffers
        del r
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        print(f"kernel {n}^2 {label}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
              f"{n * n / ms / 1e6:7.2f} Gpx/s", flush=True)

    cur = flow.copy()
    for dtype in (np.uint8, np.uint16, np.float32):
        host, full = image(n, dtype)
        mov = ctx.to_f32(ctx.asdevice(np.ascontiguousarray(np.roll(host, 1, 1))))
        ref = ctx.asdevice(host)
        del host
        warped = ctx.warp_affine_flow(mov, flow, identity)
        if dtype is np.float32:
            report("warp_affine_flow float32, linear (before every step)      ", lambda: ctx.warp_affine_flow(mov, flow, identity))
        del mov
        floor = 1e-4 * full * full
        cases = [(windows[0], None)] if dtype is not np.float32 else [(win, m) for win in windows for m in (None, keep)]
        for (name, taps), mask in cases:
            report(f"flow_refine_step {np.dtype(dtype).name:7s} {name} {'u8 mask  ' if mask is not None else 'no weight'}        ",
                   lambda t=taps, m=mask: ctx.flow_refine_step(ref, warped, cur, t, floor, m, out=cur))
        if dtype is np.float32:
            _, info = ctx.flow_refine_step(ref, warped, flow, windows[0][1], floor, return_info=True)
            print(f"one step at sigma 4 from flow B / 25: {info}", flush=True)
            for name, taps in windows:
                report(f"texture_maps     float32 {name} eigenvalues (yardstick)     ", lambda t=taps: ctx.texture_maps(ref, t))
        del ref, warped
    for name, taps in windows:
        report(f"smooth_flow all, no weight {name} (yardstick)          ", lambda t=taps: ctx.smooth_flow(flow, t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", help="a built checkout of the parent commit, benchmarked in turns with this tree")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--step", choices=["kernel"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a)
    run([sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--reps", str(a.reps), "--step", "kernel"], 500)
    if a.no_bench:
        return
    bench = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
    for _ in range(2):
        run(bench, 300)
        if a.parent:
            run(bench, 300, cwd=os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
