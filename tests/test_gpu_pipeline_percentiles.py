"""-m gpu: `python -m microaligner_amd config.yaml` with NormalizePercentiles under OptFlowReg on small .npy stacks, one hot
pixel planted in the moving cycle's reference channel: the written stack equals the same chain called by hand with
max_project_and_normalize(percentiles=(0, 99.9)), bit for bit; a run without the keys equals the chain as it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from microaligner_amd import OptFlowRegistrator, Warper, max_project_and_normalize, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = dict(NumberPyramidLevels=2, NumberIterationsPerLevel=3, TileSize=150, Overlap=30, NumberOfWorkers=0,
           UseFullResImage=True, UseDOG=False)
H, W = 300, 260


def make_cycles(tmp_path):
    ref, mov = synthetic.make_pair(H, W, seed=52, dtype=np.uint16)
    ref, mov = (ref >> 4).astype(np.uint16), (mov >> 4).astype(np.uint16)      # 12 bits of signal in a 16-bit container ...
    mov[H // 3, W // 2] = 65535                                                # ... and the hot pixel
    cycles = [np.stack([np.stack([ref, (ref // 2).astype(np.uint16)]), np.stack([(ref // 3).astype(np.uint16), ref[::-1].copy()])]),
              np.stack([np.stack([mov, (mov // 2).astype(np.uint16)]), np.stack([(mov // 3).astype(np.uint16), mov[::-1].copy()])])]
    for k, st in enumerate(cycles):
        np.save(tmp_path / f"cyc{k + 1}.npy", st)
    return cycles


def run_cli(tmp_path, name, **keys):
    cfg = {"Input": {"InputImagePaths": {f"Cycle {k}": str(tmp_path / f"cyc{k}.npy") for k in (1, 2)}, "ReferenceCycle": 1,
                     "ReferenceChannel": "0"},
           "Output": {"OutputDir": str(tmp_path / name), "OutputPrefix": "exp_", "SaveOutputToCycleStack": True},
           "RegistrationParameters": {"OptFlowReg": dict(REG, **keys)}}
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, "-m", "microaligner_amd", str(path)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(tmp_path / name / "exp_optflow_reg_result_stack.npy"), r.stdout


def chain_by_hand(cycles, **norm):
    """run_optflow_reg's steps for two cycles: the warped pages of the second."""
    reg = OptFlowRegistrator()
    reg.num_pyr_lvl, reg.num_iterations, reg.tile_size, reg.overlap, reg.use_full_res_img, reg.use_dog = 2, 3, 150, 30, True, False
    reg.ref_img = max_project_and_normalize(cycles[0][0], on_device=True, **norm)
    reg.mov_img = max_project_and_normalize(cycles[1][0], on_device=True, **norm)
    flow = reg.register()
    w = Warper()
    w.tile_size, w.overlap, w.flow = 150, 30, flow
    pages = [np.ascontiguousarray(cycles[1][c, z]) for c in range(2) for z in range(2)]
    return np.stack(w.warp_pages(pages)).reshape(2, 2, H, W)


@pytest.mark.gpu
def test_cli_normalises_by_percentiles_like_the_chain_by_hand(tmp_path):
    cycles = make_cycles(tmp_path)
    robust, log = run_cli(tmp_path, "robust", NormalizePercentiles=[0, 99.9])
    plain, plain_log = run_cli(tmp_path, "plain")
    assert robust.shape == plain.shape == (1, 4, 2, H, W) and robust.dtype == np.uint16
    assert np.array_equal(robust[0, 0:2], cycles[0]) and np.array_equal(plain[0, 0:2], cycles[0])
    assert np.array_equal(robust[0, 2:4], chain_by_hand(cycles, percentiles=(0, 99.9)))
    assert np.array_equal(plain[0, 2:4], chain_by_hand(cycles))
    # the keys are what makes the difference, and the log says what was done per cycle
    assert "NormalizePercentiles cycle 1: lo" in log and "NormalizePercentiles cycle 2: lo" in log and "saturated" in log
    assert "NormalizePercentiles" not in plain_log
    mov = cycles[1][0]
    a = max_project_and_normalize(mov, percentiles=(0, 99.9))
    b = max_project_and_normalize(mov)
    assert len(np.unique(a)) > 4 * len(np.unique(b))                # the hot pixel had squeezed the min-max image
