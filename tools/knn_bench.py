"""Micro-benchmark of ured_hip.nn.knn against what a user did before it existed,
torch.cdist(p1, p2).pow(2).topk(K, largest=False), on the same GPU in the same run.

  python tools/knn_bench.py [--iters 20] [--rounds 9] [--out FILE.json]

Per leg: both versions are warmed up, then timed in alternating rounds of `iters` calls between
two device events; the figure is the median round (min and max beside it). The K = 1 leg also
times nn_dense (both directions) on the same input. The shader clock is noted when the runtime
reports one. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.add_pkg_path()
from ured_hip import nn as unn  # noqa: E402

LEGS = [(16, 2048, 2048, 8), (16, 2048, 2048, 32), (1, 2048, 2048, 1024), (16, 2048, 2048, 1)]


def _round(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def measure(fns, iters, rounds, warm=5):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):                        # alternate the versions
        for k, fn in fns.items():
            times[k].append(_round(fn, iters))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


def _clock():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: no GPU (rates are measured on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "clock_mhz_before": _clock(), "iters": a.iters,
           "rounds": a.rounds, "legs": {}}
    for (B, n, m, K) in LEGS:
        p1 = torch.rand(B, n, 3, generator=g).to(dev)
        p2 = torch.rand(B, m, 3, generator=g).to(dev)
        fns = {"knn": lambda: unn.knn(p1, p2, K),
               "cdist_topk": lambda: torch.cdist(p1, p2).pow(2).topk(K, largest=False)}
        if K == 1:
            fns["nn_dense"] = lambda: unn.nn_dense(p1, p2)
        r = measure(fns, a.iters, a.rounds)
        # how far the baseline's answer is from ours (it uses the expansion formula)
        d, i = unn.knn(p1, p2, K)
        bd, bi = torch.cdist(p1, p2).pow(2).topk(K, largest=False)
        r["rows_with_other_indices"] = int((bi != i).any(-1).sum())
        r["rows"] = B * n
        r["gpair_s"] = B * n * m / r["knn"]["median_us"] / 1e3
        res["legs"][f"{B}x{n}x{m} K={K}"] = r
        print(f"{B}x{n}x{m} K={K}: " + "  ".join(f"{k} {v['median_us']:.1f} us ({v['min_us']:.1f}-{v['max_us']:.1f})"
                                                  for k, v in r.items() if isinstance(v, dict)), flush=True)
    res["clock_mhz_after"] = _clock()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
