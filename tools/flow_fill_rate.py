"""Rate of the push-pull fill of a flow (Context.fill_flow), include/microaligner_flowfill.h.

    python tools/flow_fill_rate.py [--size N] [--reps K] [--parent DIR] [--no-prof] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident flow -- the test suite's smooth flow B of up to 25 px -- with 5 % of the
   pixels dropped in 64 x 64 blocks and one hole a quarter of the side wide (4096 px at 16384).  Per case the median of `reps`
   HIP-event timings of one call after a warm-up call, with minimum and maximum: no weight (the dropped pixels are NaN in
   the flow), a uint8 mask, a float32 weight (the mask, soft on a tenth of the kept pixels) and a per-cell weight (64 x 64
   cells).  The bytes are those the stored form moves, counted per pixel of the flow: the first pull reads 8 + the weight
   and writes 16 / 4; the pulls above read 16 / 3 and write 16 / 12; the pushes above read 16 / 3 + 16 / 12 and write 8 / 3;
   the last push reads 8 + the weight + 16 / 4 and writes 8 -- 48 B/px and the weight twice.  Context.compose_flows on the
   same box is the yardstick.
2. prof: step 1 once more under `rocprofv3 --kernel-trace --stats`: the kernels' own times, largest launches first.
3. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from flow_smooth_rate import block_mask, device_ms, flow_b, run  # noqa: E402

CELL = 64


def holed_mask(n):
    """keep (n, n) uint8: 5 % dropped in CELL x CELL blocks and one square hole of about n / 4 a side, on the cell grid"""
    keep = block_mask(n, share=0.05, block=CELL)
    side = max(CELL, n // 4 // CELL * CELL)
    at = (n - side) // 2 // CELL * CELL
    keep[at:at + side, at:at + side] = 0
    return keep, side


def step_kernel(a):
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    keep, side = holed_mask(n)
    f = flow_b(n)
    d = ctx.asdevice(f)
    for y0 in range(0, n, 1024):
        f[y0:y0 + 1024][keep[y0:y0 + 1024] == 0] = np.nan
    d_nan = ctx.asdevice(f)
    del f
    soft = keep.astype(np.float32)
    rng = np.random.default_rng(1)
    for y0 in range(0, n, 1024):
        band = soft[y0:y0 + 1024]
        band[rng.random(band.shape, dtype=np.float32) < 0.1] *= np.float32(0.5)
    cells = np.ascontiguousarray(keep[::CELL, ::CELL]).astype(np.float32)
    cases = (("no weight      ", d_nan, None, None, 0), ("u8 mask        ", d, ctx.asdevice(keep), None, 1),
             ("f32 weight     ", d, ctx.asdevice(soft), None, 4), ("per-cell weight", d, ctx.asdevice(cells), CELL, 0))
    print(f"flow {n}^2, {100 * float((keep == 0).mean()):.1f} % dropped, hole {side} px wide", flush=True)
    for name, flow, w, cell, wbytes in cases:
        fn = lambda flow=flow, w=w, cell=cell: ctx.fill_flow(flow, w, cell)      # noqa: E731
        out, info = ctx.fill_flow(flow, w, cell, return_info=True)               # first launch, the buffers
        del out
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        bpp = 48 + 2 * wbytes
        floor_ms = bpp * n * n / 8e12 * 1e3
        print(f"kernel {n}^2 fill_flow {name}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
              f"{n * n / ms / 1e6:7.2f} Gpx/s, {bpp} B/px = {bpp * n * n / ms / 1e9:6.2f} TB/s, "
              f"{100 * floor_ms / ms:5.1f} % of 8 TB/s; {info}", flush=True)
    fn = lambda: ctx.compose_flows(d, d)                                          # noqa: E731
    res = fn()
    del res
    ms, lo, hi = device_ms(ctx, fn, a.reps)
    print(f"kernel {n}^2 compose_flows (yardstick, 24 B/px): {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}), "
          f"{24 * n * n / ms / 1e9:6.2f} TB/s", flush=True)


def prof_stats(out):
    """calls, average and total time of the fill's kernels from the profile (rocpd database, or the CSV of older rocprofv3
    versions)"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        c = sqlite3.connect(path)
        rows += c.execute("select name, count(*), avg(end - start) from kernels group by name").fetchall()
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        rows += [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]
    for name, calls, avg_ns in sorted(rows, key=lambda r: -r[1] * r[2]):
        if "ff_" in name or "compose_flows" in name:
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
            a.out = tempfile.mkdtemp(prefix="flow_fill_prof_")
        print(f"profile: {a.out}", flush=True)
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "flow_fill", "--"] + me, 500)
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
