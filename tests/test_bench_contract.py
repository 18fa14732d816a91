"""bench.py driver-contract tests: single-process and torchrun world=2 (gloo).

The round driver launches `python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...` — this must
produce exactly ONE JSON line from rank 0 with the contract fields.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse_json_line(stdout: str) -> dict:
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected exactly one JSON line, got: {stdout!r}"
    return json.loads(lines[0])


REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"]


@pytest.mark.timeout(600)
def test_bench_single_process_contract():
    out = subprocess.run(
        [sys.executable, "bench.py", "--model", "tiny", "--sidelength", "16",
         "--batch", "2", "--steps", "2", "--warmup", "1"],
        cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _parse_json_line(out.stdout)
    for k in REQUIRED:
        assert k in rec, k
    assert rec["n_gpus"] == 1
    assert rec["value"] > 0
    assert rec["scaling"] == "weak"
    assert rec["config"]["global_batch"] == 2


def _run_bench_dump(out_dir, steps, extra=()):
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--model", "tiny",
         "--sidelength", "16", "--batch", "2", "--steps", str(steps),
         "--warmup", "1", "--dump-outputs", str(out_dir), *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _parse_json_line(out.stdout)
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f))
              for f in sorted(os.listdir(out_dir))}
    return rec, arrays


@pytest.mark.timeout(600)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float32 .npy;
    the same arguments give the same inputs, so (on the deterministic CPU
    path) the same arrays; --steps really sets the number of timed steps,
    so one step more gives other parameters. --full keeps working."""
    rec_a, a = _run_bench_dump(tmp_path / "a", 2)
    rec_b, b = _run_bench_dump(tmp_path / "b", 2, extra=("--full",))
    rec_c, c = _run_bench_dump(tmp_path / "c", 3)
    assert set(a) == {"loss", "model_out", "params", "grads"}
    assert set(b) == set(a) and set(c) == set(a)
    total = 0
    for name, arr in a.items():
        assert arr.dtype == np.float32, name
        assert np.isfinite(arr).all(), name
        assert arr.shape == b[name].shape == c[name].shape, name
        total += arr.nbytes
    assert total <= 64 * 1024 * 1024
    assert a["model_out"].shape == (2, 16, 16, 3)  # channels-last images
    assert a["params"].size == rec_a["config"]["params"]
    assert float(a["loss"]) == pytest.approx(rec_a["config"]["final_loss"])
    if rec_a["dtype"] == "fp32":  # CPU path is bit-reproducible; GPU kernels
        for name in a:            # that accumulate with atomics are not
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert rec_a["steps"] == 2 and rec_c["steps"] == 3
    assert rec_a["ms_per_step"] > 0
    assert not np.array_equal(a["params"], c["params"])


@pytest.mark.timeout(900)
def test_bench_torchrun_world2_contract():
    env = dict(os.environ)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    if torch.cuda.device_count() < 2:
        # one rank per GPU needs 2 GPUs; with fewer, hide them from the
        # ranks so both take the CPU/gloo path (the contract is the same)
        env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = "-1"
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29517", "bench.py", "--gpus", "2",
         "--model", "tiny", "--sidelength", "16", "--batch", "2",
         "--steps", "2", "--warmup", "1"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=840)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = _parse_json_line(out.stdout)
    assert rec["n_gpus"] == 2
    assert rec["config"]["global_batch"] == 4  # 2 per rank x 2 ranks
    assert rec["config"]["parallelism"] == "dp2"
