"""bench.py: a plain run does only what its headline needs; --full adds everything measured or checked beside it."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a plain line carries beyond the headline: no key of --full's measurements
FULL_ONLY = ("variants", "cpu_baseline", "roofline", "roofline_blur_v", "roofline_polyexp", "roofline_blur_h_solve",
             "sustained_clock_ghz", "results_to_shared_array", "results_to_shared_array_ms", "host_modes")


def _bench(*args, timeout=600, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_multi_rank_dry_run_leaves_the_host_modes_to_full():
    """`--gpus N` without --full: the ranks rendezvous, time and reduce as before, and no host mode runs."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    res = _bench("--gpus", "2", "--steps", "2", "--warmup", "0", "--dry-run", env=env)
    assert res["n_gpus"] == 2 and res["steps"] == 2 and [row["rank"] for row in res["ranks"]] == [0, 1]
    assert res["host_modes"] is None
    # asked for by name, the modes run without --full
    res = _bench("--gpus", "2", "--steps", "2", "--warmup", "0", "--dry-run", "--host-modes", "on", env=env)
    assert set(res["host_modes"]) >= {"stream_pairs_pageable", "warp_pages_page_locked"}


@pytest.mark.gpu
def test_plain_and_full_lines():
    """The same small workload plain and with --full: the headline fields of both, the informational legs, CPU baseline,
    clock probe and roofline only in the second, each without an error."""
    plain = _bench("--workload", "cfg1", "--steps", "2", "--warmup", "1")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "kernels", "step_ms_host"):
        assert k in plain, k
    assert plain["steps"] == 2 and plain["warmup"] == 1 and len(plain["step_ms_host"]) == 2
    assert plain["value"] > 0 and plain["higher_is_better"] is True and plain["kernels"]
    assert not [k for k in FULL_ONLY if k in plain]
    assert "clock_ghz" not in plain["ranks"][0]

    full = _bench("--workload", "cfg1", "--steps", "2", "--warmup", "1", "--full")
    assert {k: full[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup")} == \
        {k: plain[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup")}
    assert full["value"] > 0 and full["sustained_clock_ghz"] > 0 and full["ranks"][0]["clock_ghz"] > 0
    assert full["roofline"]["kernel"] in full["kernels"]
    assert full["cpu_baseline"]["value"] > 0, full["cpu_baseline"]
    V = full["variants"]
    assert set(V) >= {"host_inclusive", "host_stream", "host_stream_u8", "muladd_fma", "page_warp", "lanes3"}, V
    assert not [k for k, v in V.items() if "error" in v], V
