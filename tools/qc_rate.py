"""Rate of the registration quality maps on a device-resident 16384^2 float32 pair with its flow.

    python tools/qc_rate.py [size] [--cell N] [--reps K]

Times assess_registration() end to end (wall clock, inputs already in HBM) and the two passes of csrc/qc.hip alone through
the library's per-kernel accounting (ma_profile_*, HIP events around the launches): the flow pass (ma_qc_flow_grid, 8 B/px)
and the histogram pass (ma_qc_nmi_grid over the reference and two label images, 3 B/px).  Rates are HBM bytes the pass must
read over its time, against the MI355X's 8 TB/s peak."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from microaligner_amd import assess_registration
from microaligner_amd.device import get_context

PEAK = 8.0e12


def profiled_ms(ctx, fn, reps):
    """Median over `reps` calls of the library's own accounting of the launches of one call."""
    out = []
    for _ in range(reps):
        ctx.profile_reset()
        fn()
        out.append(ctx.profile_get()["other"]["ms"])
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=16384)
    ap.add_argument("--cell", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    H = W = a.size
    rng = np.random.default_rng(0)
    y = np.arange(H, dtype=np.float32)[:, None]
    x = np.arange(W, dtype=np.float32)[None, :]
    ref = (127.0 + 50.0 * np.sin(x * 0.011) * np.cos(y * 0.007) + rng.standard_normal((H, W), dtype=np.float32) * 20.0)
    ref = ref.astype(np.float32)
    mov = np.roll(ref, (3, -2), axis=(0, 1))
    flow = np.empty((H, W, 2), np.float32)
    flow[..., 0] = -2.0 + 0.5 * np.sin(y * 0.003)
    flow[..., 1] = 3.0 + 0.5 * np.cos(x * 0.002)
    ctx = get_context()
    d_ref, d_mov, d_flow = ctx.asdevice(ref), ctx.asdevice(mov), ctx.asdevice(flow)
    del ref, mov, flow
    ctx.sync()

    qc = assess_registration(d_ref, d_mov, d_flow, cell_size=a.cell)      # warm-up: workspace, buffers, code objects
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        qc = assess_registration(d_ref, d_mov, d_flow, cell_size=a.cell)
        walls.append((time.perf_counter() - t0) * 1e3)
    s = qc.summary()
    print(f"assess_registration {H}x{W} f32, cells of {a.cell} ({s['cells']}): {np.median(walls):.2f} ms median wall "
          f"(min {min(walls):.2f}); cells improved {s['cells_improved']}, folded {s['folded']}, invalid {s['invalid']}")

    wrp = ctx.warp(d_mov, d_flow, 1000, 100)
    labels = [ctx.dog_u8(v) for v in (d_ref, wrp, d_mov)]
    ctx.sync()
    ctx.profile(True)
    try:
        flow_ms = profiled_ms(ctx, lambda: ctx.qc_flow_grid(d_flow, a.cell, a.cell), a.reps)
        nmi_ms = profiled_ms(ctx, lambda: ctx.qc_nmi_grid(labels[0], labels[1], labels[2], a.cell, a.cell), a.reps)
    finally:
        ctx.profile(False)
    fb, nb = 8.0 * H * W, 3.0 * H * W
    print(f"flow pass (ma_qc_flow_grid): {flow_ms:.3f} ms, {fb / 1e9:.2f} GB -> {fb / flow_ms / 1e6:.0f} GB/s "
          f"= {100 * fb / flow_ms * 1e3 / PEAK:.0f}% of 8 TB/s")
    print(f"histogram pass (ma_qc_nmi_grid, 2 label images): {nmi_ms:.3f} ms, {nb / 1e9:.2f} GB -> {nb / nmi_ms / 1e6:.0f} GB/s "
          f"= {100 * nb / nmi_ms * 1e3 / PEAK:.0f}% of 8 TB/s, {2.0 * H * W / nmi_ms / 1e6:.0f} Gpx-pairs/s")


if __name__ == "__main__":
    main()
