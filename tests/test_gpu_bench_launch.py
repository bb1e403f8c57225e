"""bench.py --gpus N starts its own ranks (no external launcher): the parent never
touches the GPU and spawns N fresh rank processes. Rehearsed here with the gloo backend
on the box's one GPU (TT_DIST_BACKEND=gloo; the 8-GPU node runs the same code over
RCCL). Checks the driver contract: exactly one JSON line, from rank 0, n_gpus = N,
whole-job value, finite losses."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("loss", ["hardneg_margin", "infonce"])
def test_bench_spawns_two_ranks_without_launcher(loss):
    env = dict(os.environ, TT_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "512", "--vocab", "20000", "--loss", loss, "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["parallelism"] == "dp2"
    assert rec["config"]["global_batch"] == 1024
    assert rec["value"] > 0 and all(abs(x) < 1e3 for x in rec["loss_first_last"])


def _run_bench(*flags):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TT_DIST_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch", "512", "--vocab", "20000", *flags]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_bench_prints_headline_only_and_dumps_last_step(tmp_path):
    """A plain run carries the headline fields and none of the --full measurements;
    --dump-outputs writes the last timed step's loss, both towers' vectors and every
    updated parameter as finite float32 arrays."""
    import numpy as np
    rec = _run_bench("--dump-outputs", str(tmp_path / "dump"))
    assert rec["steps"] == 2 and rec["unit"] == "pairs/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] * 1e-3 / 512 - 1) < 1e-3
    for k in ("roofline", "rooflines_secondary", "kernel_ms_per_step", "cpu_baseline"):
        assert k not in rec, k
    files = {f: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert {"loss.npy", "query_vectors.npy", "doc_vectors.npy", "param.query_proj.0.weight.npy"} <= set(files)
    assert len(files) == 3 + 44  # the 44 state_dict keys
    assert files["query_vectors.npy"].shape == files["doc_vectors.npy"].shape == (512, 256)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert abs(float(files["loss.npy"]) - rec["loss_first_last"][1]) < 1e-4
    assert sum(a.nbytes for a in files.values()) <= 64 * 10**6


def test_full_bench_adds_rooflines_and_cpu_baseline():
    """--full keeps the headline and adds the HIP-event figures of the timed steps and the
    reference CPU baseline (a one-step sample here)."""
    rec = _run_bench("--full", "--cpu-batch", "32", "--cpu-steps", "1", "--cpu-warmup", "0")
    assert rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["roofline"]["kernel"] and rec["roofline"]["region"] in rec["kernel_ms_per_step"]
    assert rec["rooflines_secondary"] and "gru_fwd" in rec["kernel_ms_per_step"]
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["kind"] == "reference"
