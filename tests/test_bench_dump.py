"""bench.py --dump-outputs: what the timed path computed, written as .npy for an output-for-output comparison of two builds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_stays_under_the_limit_with_a_fixed_sample(tmp_path, monkeypatch):
    """Images that fit are written whole; larger ones at the same seeded pixel positions in every image and every run, all
    files float32 / float64 and together within DUMP_LIMIT_BYTES."""
    assert bench.DUMP_LIMIT_BYTES <= 64 * 10 ** 6
    rng = np.random.default_rng(3)
    flow = rng.standard_normal((300, 280, 2), dtype=np.float32)
    warped = rng.integers(0, 256, (300, 280), dtype=np.uint8)
    levels = np.array([[4, 0.5, 0.4, 1], [1, 0.6, 0.5, 0]], np.float64)

    whole = bench.dump_outputs(str(tmp_path / "whole"), {"flow": flow, "warped": warped}, {"levels": levels})
    got = _load_dir(tmp_path / "whole")
    assert whole["sample"] is None and set(got) == {"flow", "warped", "levels"}
    assert got["flow"].dtype == np.float32 and np.array_equal(got["flow"], flow)
    assert got["warped"].dtype == np.float32 and np.array_equal(got["warped"], warped.astype(np.float32))
    assert got["levels"].dtype == np.float64 and np.array_equal(got["levels"], levels)

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    runs = []
    for k in range(2):
        d = tmp_path / f"sampled{k}"
        info = bench.dump_outputs(str(d), {"flow": flow, "warped": warped}, {"levels": levels})
        runs.append(_load_dir(d))
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= bench.DUMP_LIMIT_BYTES
    n = info["sample"]["pixels"]
    assert 0 < n < 300 * 280 and runs[0]["flow"].shape == (n, 2) and runs[0]["warped"].shape == (n,)
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(300 * 280, size=n, replace=False))
    assert np.array_equal(runs[0]["flow"], flow.reshape(-1, 2)[pos])
    assert np.array_equal(runs[0]["warped"], warped.reshape(-1)[pos].astype(np.float32))


def test_bench_rejects_a_step_count_below_one():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_what_the_oracle_computes(tmp_path):
    """The files of `bench.py --workload cfg1 --dump-outputs DIR` are the last step's flow, warped image and level reports of
    pair 0, and equal the CPU oracle's register() + warp() of the same seeded pair; --steps sets the timed steps."""
    from microaligner_amd import synthetic
    from oracle import register_oracle as RO
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg1", "--steps", "2", "--warmup", "1",
                        "--no-variants", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == 2 and len(res["step_ms_host"]) == 2
    assert res["dump_outputs"]["sample"] is None
    got = _load_dir(tmp_path)
    assert set(got) == {"flow", "warped", "levels"}

    H, W = bench.WORKLOADS["cfg1"]["shape"]
    ref, mov = synthetic.make_pair(H, W, seed=1)
    exp_flow, reports = RO.register(ref, mov)
    assert np.array_equal(got["flow"], exp_flow)
    assert np.array_equal(got["warped"], RO.warp(mov, exp_flow, 1000, 100))
    assert [(f, a) for f, _, _, a in got["levels"]] == [(r[0], r[3]) for r in reports]
    np.testing.assert_allclose(got["levels"][:, 1:3], [r[1:3] for r in reports], rtol=0, atol=1e-12)
