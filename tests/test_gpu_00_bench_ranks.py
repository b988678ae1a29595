"""`bench.py --gpus N` on the GPU (config C4's launcher path): without a
launcher it starts its own N ranks (torch.distributed.run, one process per
GPU), refuses more ranks than visible GPUs, and with --allow-shared (a
rehearsal of N ranks on one GPU) gathers every rank's tile ImageBlocks to
rank 0 and, under --full, checks the assembled frame against a whole-frame
render and runs the parity leg on it; a plain run only times its steps and
can dump its last frame (--dump-outputs).  This file runs first among the GPU tests (its name sorts
first) and never initialises the GPU in the pytest process itself: the ranks
are child processes, and a process that has initialised the GPU must not
start programs (the device count here comes from torch, which does not
initialise it)."""
import json
import os
import subprocess
import sys

import pytest

import bench
from conftest import REPO

pytestmark = pytest.mark.gpu


def _bench(args, timeout=600):
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, cwd=REPO)


SMALL = ["--workload", "cbox", "--width", "320", "--height", "180", "--spp", "16", "--steps", "2", "--warmup", "1",
         "--no-cpu"]


def test_bench_two_ranks_gather_and_check_the_frame():
    r = _bench(["--gpus", "2", "--allow-shared", "--full", *SMALL])   # --full: the assembly check and the parity leg
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["devices"]["distinct"] >= 1 and len(out["devices"]["pci"]) == 2
    assert out["assembly"]["pass"], out["assembly"]
    assert out["parity"]["pass"], out["parity"]
    assert "assembled from all 2 ranks" in out["parity"]["tiles"]


def test_plain_run_times_its_steps_and_dumps_the_frame(tmp_path):
    """Without --full the run only times its steps (no roofline, parity or
    CPU-baseline leg) and --dump-outputs writes the last frame's ImageBlock."""
    import numpy as np
    r = _bench(["--gpus", "1", "--dump-outputs", str(tmp_path / "out"), *SMALL], timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    # value = the frame's samples over one timed step's time; the line rounds
    # ms_per_step to 0.01 ms (half a unit either way) and value to 0.001
    ms = out["ms_per_step"]
    assert out["value"] == pytest.approx(320 * 180 * 16 / (ms * 1e-3) / 1e6, rel=0.005 / (ms - 0.005) + 1e-4)
    assert out["roofline"] is None and out["parity"] is None and out["cpu_baseline"] is None
    assert out["kernels"]["frame_ms"] > 0 and "pmc" not in out["kernels"]
    assert sorted(os.listdir(tmp_path / "out")) == ["imageblock.npy"]
    block = np.load(tmp_path / "out" / "imageblock.npy")
    assert block.dtype == np.float32 and block.ndim == 3 and block.shape[2] == 5
    assert block.shape[0] > 180 and block.shape[1] > 320 and block.shape[0] - 180 == block.shape[1] - 320
    b = (block.shape[0] - 180) // 2
    weight = block[b:-b, b:-b, 4]
    assert np.isfinite(block).all() and (weight > 0).all() and block[b:-b, b:-b, :3].mean() > 0


@pytest.mark.skipif(bench.visible_gpus() >= 2, reason="needs a box with fewer than 2 GPUs")
def test_bench_refuses_two_ranks_on_one_gpu():
    r = _bench(["--gpus", "2", *SMALL], timeout=300)
    assert r.returncode != 0
    assert "refusing" in r.stderr, r.stderr[-2000:]
    assert not [line for line in r.stdout.splitlines() if line.startswith("{")]
