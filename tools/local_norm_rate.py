"""Rate of the local contrast normalisation (Context.normalize_local), include/microaligner_localnorm.h.

    python tools/local_norm_rate.py [--size N] [--reps K] [--parent DIR] [--no-prof] [--no-bench] [--out DIR]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident uint16 image (the pattern of tools/texture_rate.py, a quarter of it
   exactly constant), uint8 output.  Per case the median of `reps` HIP-event timings of one call after a warm-up call, with
   minimum and maximum: sigma 4 (r = 12) and sigma 16 (r = 48), each without a weight and with a uint8 mask that drops 1 %
   of the image in blocks of 64; then the counts of one call.  The yardstick on the same box with the same taps:
   Context.local_correlation (score plane) of the image and a float32 copy of it -- six planes in two passes against
   three plane-passes in two stages.
2. prof: step 1 once more under `rocprofv3 --kernel-trace --stats`: the kernels' own times, largest first.
3. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from flow_smooth_rate import block_mask, device_ms, run
from texture_rate import image


def step_kernel(a):
    from microaligner_amd.device import gaussian_taps, get_context
    ctx = get_context()
    n = a.size
    windows = (("sigma 4 (r 12) ", gaussian_taps(4.0)), ("sigma 16 (r 48)", gaussian_taps(16.0)))
    assert [len(t) - 1 for _, t in windows] == [12, 48]
    host, full = image(n, np.uint16)
    d_img = ctx.asdevice(host)
    del host
    keep = ctx.asdevice(block_mask(n))
    floor = 6.4e-5 * full * full
    for name, taps in windows:
        for label, weight in (("no weight ", None), ("uint8 mask", keep)):
            fn = lambda t=taps, w=weight: ctx.normalize_local(d_img, t, floor, 4.0, w)       # noqa: E731
            r = fn()                                        # first launch, the buffers
            del r
            ms, lo, hi = device_ms(ctx, fn, a.reps)
            print(f"kernel {n}^2 normalize_local uint16 -> uint8 {name} {label}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, "
                  f"{a.reps} calls), {n * n / ms / 1e6:7.2f} Gpx/s", flush=True)
    _, info = ctx.normalize_local(d_img, windows[0][1], floor, 4.0, keep, return_info=True)
    print(f"counts at floor 6.4e-5 of squared full scale, clip 4: {info} of {n * n}", flush=True)
    d_f32 = ctx.to_f32(d_img)
    for name, taps in windows:
        fn = lambda t=taps: ctx.local_correlation(d_img, d_f32, t, floor, (0.5 * full, 0.5 * full))      # noqa: E731
        r = fn()
        del r
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        print(f"kernel {n}^2 local_correlation uint16, score     {name} (yardstick): {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, "
              f"{a.reps} calls), {n * n / ms / 1e6:7.2f} Gpx/s", flush=True)


def prof_stats(out):
    """calls, average and total time of the kernels of both calls from the profile (rocpd database, or the CSV of older
    rocprofv3 versions)"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        c = sqlite3.connect(path)
        rows += c.execute("select name, count(*), avg(end - start) from kernels group by name").fetchall()
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        rows += [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]
    for name, calls, avg_ns in sorted(rows, key=lambda r: -r[1] * r[2]):
        if "ln_" in name or "lc_" in name or "wf_setup" in name:
            print(f"  {avg_ns / 1e6:8.4f} ms avg  {calls:4d} calls  {calls * avg_ns / 1e6:9.3f} ms in all  {name[:100]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", help="a built checkout of the parent commit, benchmarked in turns with this tree")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", help="directory of the profile (default: a new temporary directory)")
    ap.add_argument("--step", choices=["kernel"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a)
    me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--reps", str(a.reps), "--step", "kernel"]
    run(me, 500)
    if not a.no_prof:
        if not a.out:
            import tempfile
            a.out = tempfile.mkdtemp(prefix="local_norm_prof_")
        print(f"profile: {a.out}", flush=True)
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "local_norm", "--"] + me, 500)
        prof_stats(a.out)
    if a.no_bench:
        return
    bench = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
    for _ in range(2):
        run(bench, 300)
        if a.parent:
            run(bench, 300, cwd=os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
