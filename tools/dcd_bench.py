"""Times calc_dcd(x, gt, alpha, n_lambda)[0].sum().backward() through the fused Function
(ured_hip.dcd: NN + one reduction launch forward, one launch backward) against the torch tail on the
NN Function that calc_dcd used before it (about a dozen elementwise / scatter / gather launches each
way plus ured_nn_bwd_set), on the same GPU in the same run.

  python tools/dcd_bench.py [--iters 20] [--rounds 9] [--out FILE.json]

Legs: B x n_x x n_gt = 32 x 2048 x 2048 and 32 x 1024 x 2048, each with (alpha, lambda) = (1000, 1) and
(200, 0.5). Per leg both versions are warmed up, then timed in alternating rounds of `iters` calls
between two device events; the figure is the median round (min and max beside it). The two versions'
losses and gradients are compared once per leg. Run the command twice for the run-to-run spread.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [(32, 2048, 2048, 1000, 1), (32, 2048, 2048, 200, 0.5), (32, 1024, 2048, 1000, 1), (32, 1024, 2048, 200, 0.5)]


def torch_tail(x, gt, alpha=1000, n_lambda=1):
    """calc_dcd as it ran under autograd before the fused Function: calc_cd on the NN Function, then
    the reference's elementwise / scatter / gather tail (model_utils.py:27-45)."""
    import torch
    from chamfer3D.model_utils import calc_cd
    n_x, n_gt = x.shape[1], gt.shape[1]
    cd_p, cd_t, dist1, dist2, idx1, idx2 = calc_cd(x, gt, return_raw=True)
    exp1, exp2 = torch.exp(-dist1 * alpha), torch.exp(-dist2 * alpha)
    cnt1 = torch.zeros_like(idx2).scatter_add_(1, idx1.long(), torch.ones_like(idx1))
    w1 = (cnt1.gather(1, idx1.long()).float().detach() ** n_lambda + 1e-6) ** (-1) * (n_gt / n_x)
    cnt2 = torch.zeros_like(idx1).scatter_add_(1, idx2.long(), torch.ones_like(idx2))
    w2 = (cnt2.gather(1, idx2.long()).float().detach() ** n_lambda + 1e-6) ** (-1) * (n_x / n_gt)
    return [((1 - exp1 * w1).mean(dim=1) + (1 - exp2 * w2).mean(dim=1)) / 2, cd_p, cd_t]


def _round(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from chamfer3D import model_utils as M
    if not torch.cuda.is_available():
        raise SystemExit("dcd_bench: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"iters": a.iters, "rounds": a.rounds, "legs": {}}
    for b, n_x, n_gt, alpha, lam in LEGS:
        x = (torch.rand(b, n_x, 3, generator=g) ** 2).to(dev).requires_grad_(True)
        gt = torch.rand(b, n_gt, 3, generator=g).to(dev)

        def step(fn):
            x.grad = None
            loss = fn(x, gt, alpha=alpha, n_lambda=lam)[0]
            loss.sum().backward()
            return loss.detach(), x.grad

        fns = {"fused": lambda: step(M.calc_dcd), "torch_tail": lambda: step(torch_tail)}
        (l0, g0), (l1, g1) = fns["fused"](), fns["torch_tail"]()
        leg = {"loss_max_abs_diff": float((l0 - l1).abs().max()),
               "grad_max_abs_diff": float((g0 - g1).abs().max()), "grad_max_abs": float(g1.abs().max())}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.rounds):                  # alternate the versions
            for k, fn in fns.items():
                times[k].append(_round(fn, a.iters))
        for k, v in times.items():
            leg[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
        leg["torch_over_fused"] = leg["torch_tail"]["median_us"] / leg["fused"]["median_us"]
        name = f"{b}x{n_x}x{n_gt} alpha {alpha} lambda {lam}"
        res["legs"][name] = leg
        print(f"{name}: fused {leg['fused']['median_us']:.1f} us ({leg['fused']['min_us']:.1f}-{leg['fused']['max_us']:.1f})  "
              f"torch tail {leg['torch_tail']['median_us']:.1f} us ({leg['torch_tail']['min_us']:.1f}-"
              f"{leg['torch_tail']['max_us']:.1f})  torch/fused {leg['torch_over_fused']:.2f}  "
              f"grad diff {leg['grad_max_abs_diff']:.2e} of {leg['grad_max_abs']:.2e}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
