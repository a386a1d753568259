"""bench.py's multi-rank launcher on CPU: `python bench.py --gpus 2` without torch.distributed.run
starts the two ranks itself, and the JSON line reports the world size the ranks actually formed
(--cpu-dry-run replaces the GPU step by a gloo all_reduce; the launch path is the real one)."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def test_bench_gpus2_spawns_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                        "--warmup", "1", "--cpu-dry-run"], capture_output=True, text=True, timeout=240, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["dry_run"]


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: small arrays whole, an array over its share of the budget as a sample of its
    flattened elements at indices that depend only on its name and size; the budget holds in all."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    rng = np.random.default_rng(0)
    arrs = {"out.small": rng.random(7).astype(np.float32), "out.count": np.arange(3, dtype=np.float64),
            "state.big": rng.random((50, 100)).astype(np.float32)}
    bench.dump_outputs(arrs, str(tmp_path / "a"))
    bench.dump_outputs({k: v + 1 for k, v in arrs.items()}, str(tmp_path / "b"))
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrs}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(n + ".npy" for n in arrs)
    assert np.array_equal(got["out.small"], arrs["out.small"]) and got["out.small"].dtype == np.float32
    assert np.array_equal(got["out.count"], arrs["out.count"]) and got["out.count"].dtype == np.float64
    big = got["state.big"]
    assert big.dtype == np.float32 and big.ndim == 1 and 0 < big.size < arrs["state.big"].size
    assert sum(a.nbytes for a in got.values()) <= 4096
    assert np.isin(big, arrs["state.big"]).all()
    # the same elements in the second dump (every value there is one higher)
    assert np.array_equal(np.load(tmp_path / "b" / "state.big.npy"), big + 1)
