"""Rate of the alignment moments (Context.direct_affine_moments, include/microaligner_direct.h) and of a whole
align_affine.

    python tools/direct_affine_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: N^2 (default 16384^2) device-resident pairs (uint8, uint16, float32: a texture of plane waves and the same
   texture under a small rotation and a shift of 3 px, the corners about 6 px off).  Per case the median of `reps` HIP-event timings of one call after
   a warm-up call, with minimum and maximum, and the bytes the case must move at least (the reference once, the moving image
   once, the weight's 4 B/px) over that time against the 8 TB/s peak: the pass at the identity and at a 3 degree matrix,
   with and without a float32 weight, and with a clip.  A whole align_affine (3 pyramid levels) from the identity, host
   clock around it, with its passes per level; for uint8 also under a device-resident uint8 mask, whose float32 pyramid is
   made on the device.  Yardsticks on the same box: Context.flow_affine_moments without a weight
   (the same reduction over 8 B/px) and the float32 linear Context.warp_affine (the same gather).
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_TBS = 8.0


def rotation(n, deg, shift):
    """M (reference pixels -> moving pixels): a rotation about the image's centre and a shift"""
    c = (n - 1) / 2.0
    th = math.radians(deg)
    L = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    return np.concatenate([L, (np.array([c, c]) - L @ np.array([c, c]) + np.asarray(shift, float))[:, None]], 1)


def texture(n, M, seed=3):
    """float32, four plane waves of periods 9 to 40 px evaluated at M^-1 p, over 0.15 to 0.45 of 255, built in row bands"""
    rng = np.random.default_rng(seed)
    period, ang, ph = rng.uniform(9, 40, 4), rng.uniform(0, math.pi, 4), rng.uniform(0, 2 * math.pi, 4)
    kx, ky = 2 * math.pi * np.cos(ang) / period, 2 * math.pi * np.sin(ang) / period
    Mi = np.linalg.inv(np.append(M, [[0, 0, 1]], axis=0))[:2]
    out = np.empty((n, n), np.float32)
    xx = np.arange(n, dtype=np.float64)[None, :]
    for y0 in range(0, n, 512):
        yy = np.arange(y0, min(y0 + 512, n), dtype=np.float64)[:, None]
        f = 0.0
        for u, v, p in zip(kx, ky, ph):
            # the phase of a wave is linear in (x, y): one row and one column in float64, their sum in float32
            a, b = u * Mi[0, 0] + v * Mi[1, 0], u * Mi[0, 1] + v * Mi[1, 1]
            phase = np.mod(a * xx + (u * Mi[0, 2] + v * Mi[1, 2] + p), 2 * math.pi) + np.mod(b * yy, 2 * math.pi)
            f = f + np.cos(phase.astype(np.float32))
        out[y0:y0 + 512] = (0.30 + 0.15 / 4.0 * f) * 255.0
    return out


def as_dtype(img, dtype):
    """the float32 texture in the range of dtype"""
    if dtype == np.float32:
        return img
    return np.rint(img * (np.iinfo(dtype).max / 255.0)).astype(dtype)


def device_ms(ctx, fn, reps):
    out = []
    a, b = ctx.event(), ctx.event()
    for _ in range(reps):
        ctx.record(a)
        r = fn()
        ctx.record(b)
        out.append(ctx.elapsed_ms(a, b))
        del r
    return float(np.median(out)), min(out), max(out)


def step_kernel(a):
    from microaligner_amd import align_affine
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    truth = rotation(n, 0.3 * 1024 / n, (3.0, -2.0))      # corners about 6 px off at any size
    eye, rot3 = np.eye(2, 3), rotation(n, 3.0, (0.0, 0.0))
    w32 = ctx.asdevice(np.random.default_rng(0).uniform(0.5, 1.5, (n, n)).astype(np.float32))
    w8 = ctx.asdevice((np.random.default_rng(1).random((n, n), np.float32) < 0.9).astype(np.uint8))

    def report(name, bpp, fn):
        r = fn()                                        # first launch, the buffers
        del r
        ctx.sync()
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        tbs = n * n * bpp / ms / 1e9
        print(f"kernel {n}^2 {name}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
              f"{n * n / ms / 1e6:7.2f} Gpx/s, {bpp:2d} B/px = {tbs:5.2f} TB/s = {100 * tbs / PEAK_TBS:4.1f} % of peak", flush=True)

    base_ref, base_mov = texture(n, eye), texture(n, truth)
    for dtype in (np.uint8, np.uint16, np.float32):
        name, size = np.dtype(dtype).name, np.dtype(dtype).itemsize
        ref, mov = ctx.asdevice(as_dtype(base_ref, dtype)), ctx.asdevice(as_dtype(base_mov, dtype))
        report(f"moments {name:7s} identity            ", 2 * size, lambda: ctx.direct_affine_moments(ref, mov, eye))
        report(f"moments {name:7s} 3 degrees           ", 2 * size, lambda: ctx.direct_affine_moments(ref, mov, rot3))
        report(f"moments {name:7s} identity, f32 weight", 2 * size + 4, lambda: ctx.direct_affine_moments(ref, mov, eye, weight=w32))
        report(f"moments {name:7s} 3 degrees, f32 weight", 2 * size + 4, lambda: ctx.direct_affine_moments(ref, mov, rot3, weight=w32))
        report(f"moments {name:7s} identity, clip      ", 2 * size, lambda: ctx.direct_affine_moments(ref, mov, eye, clip=0.02 * (255.0 if size == 4 else np.iinfo(dtype).max)))
        _, counts = ctx.direct_affine_moments(ref, mov, rot3)
        print(f"used / outside / invalid / unweighted / trimmed at 3 degrees: {counts.tolist()}", flush=True)
        for rep in range(2):
            ctx.sync()
            t0 = time.perf_counter()
            tmat, info = align_affine(ref, mov, "affine", return_info=True)
            dt = time.perf_counter() - t0
            M = np.linalg.inv(np.append(tmat, [[0, 0, 1]], axis=0))[:2]
            corners = np.array([[x, y, 1.0] for x in (0.0, n - 1.0) for y in (0.0, n - 1.0)])
            err = float(np.hypot(*(corners @ (M - truth).T).T).max())
            print(f"align_affine {n}^2 {name} (call {rep + 1}): {1e3 * dt:8.1f} ms, passes per level "
                  f"{[(lv.factor, lv.passes, lv.rejected) for lv in info.levels]}, accepted {info.accepted}, corner error "
                  f"{err:.4f} px, used {info.used_share:.3f}", flush=True)
        if dtype == np.uint8:
            for rep in range(2):
                ctx.sync()
                t0 = time.perf_counter()
                tmat, info = align_affine(ref, mov, "affine", weight=w8, return_info=True)
                dt = time.perf_counter() - t0
                print(f"align_affine {n}^2 {name}, uint8 mask (call {rep + 1}): {1e3 * dt:8.1f} ms, passes per level "
                      f"{[(lv.factor, lv.passes, lv.rejected) for lv in info.levels]}, accepted {info.accepted}, used "
                      f"{info.used_share:.3f}", flush=True)
        if dtype == np.float32:
            hom3 = np.append(rot3, [[0, 0, 1]], axis=0)
            report("warp_affine float32 3 degrees (yardstick)", 8, lambda: ctx.warp_affine(mov, hom3))
        del ref, mov
    flow = ctx.zeros((n, n, 2), np.float32)
    report("flow_affine_moments, no weight (yardstick)", 8, lambda: ctx.flow_affine_moments(flow))


def run(cmd, limit, cwd=ROOT):
    print("+", " ".join(cmd), f"(in {cwd})", flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd)
    if r.returncode != 0:
        print(f"step failed with status {r.returncode}: stopping", flush=True)
        sys.exit(r.returncode)


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
