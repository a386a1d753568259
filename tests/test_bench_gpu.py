"""bench.py's N > 1 path end to end on the one GPU of a test box: `--gpus 2 --dist-backend gloo`
launches two ranks through torch.distributed.run (both on GPU 0), replays the data-parallel step
as segmented HIP graphs (the contrastive all_gather between the segments, the gradient
all-reduce after them) and prints ONE JSON line with the whole-job rate. The driver's scaling
run is the same code with RCCL and one GPU per rank; the rate here means nothing."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(400)
def test_bench_two_ranks_gloo(dev):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--steps", "3",
           "--warmup", "1", "--batch", "4", "--no-extras", "--no-cpu-baseline", "--no-breakdown",
           "--no-all-slots-rate", "--no-k16-rate", "--no-loader-rate"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=360)
    assert p.returncode == 0, p.stderr[-5000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["scaling"] == "weak"
    assert d["step_mode"] == "hip_graph"
    assert d["value"] > 0 and d["config"]["global_batch"] == 8
    print(lines[0][:300])


@pytest.mark.timeout(200)
def test_bench_plain_run_dumps_outputs(dev, tmp_path):
    """A plain run (no --full) times exactly --steps steps, prints the headline line without the
    side measurements, and --dump-outputs leaves the last step's outputs and the model state."""
    import numpy as np
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "4", "--points", "512", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr[-5000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "iters/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-3
    assert d["roofline"] is None and d["cpu_baseline"] is None
    for k in ("gemm_variants", "all_slots_iters_s", "k16_iters_s", "loader", "chamfer", "inference", "emd"):
        assert k not in d, k
    files = {f.name: np.load(f) for f in out.iterdir()}
    assert "out.all_loss.npy" in files and "out.out.npy" in files
    assert any(n.startswith("state.src_encoder_all.") for n in files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert float(files["out.all_loss.npy"]) == pytest.approx(d["loss"], rel=1e-6)
    assert files["out.out.npy"].shape[0] == 4 and np.isfinite(files["out.out.npy"]).all()
