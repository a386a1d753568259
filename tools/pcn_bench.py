"""Times one PCN training step (models/pcn.py: forward, the dcd loss of the config, backward) on the
HIP Functions against the torch composition a user had before them (conv1d / linear on the
concatenated [B, C, N] operands, the same weights, the same loss), on the same GPU in the same run.

  python tools/pcn_bench.py [--iters 5] [--rounds 7] [--out FILE.json] [--batch 32]

Shape of cfgs/pcn_dcd.yaml: B 32, 2048 input points, num_coarse 1024, num_points 2048, loss dcd with
alpha 200, lambda 0.5, fine-loss weight 0.5. Both versions are warmed up, then timed in alternating
rounds of `iters` steps between two device events; the figure is the median round (min and max
beside it). Peak memory is the torch.cuda.max_memory_allocated delta of one step. Each version's
parameter gradients are compared once with those of the composition in float64. Run the command
twice for the run-to-run spread. Prints one JSON line.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_forward(m, x):
    """The reference's encoder and decoder with m's parameters -> (coarse [B,nc,3], fine [B,nf,3])."""
    import torch
    import torch.nn.functional as F
    e, d = m.encoder, m.decoder
    B, _, N = x.shape
    h = e.conv2(F.relu(e.conv1(x)))
    g = h.max(2)[0]
    h = F.relu(e.conv3(torch.cat((h, g.unsqueeze(2).expand(-1, -1, N)), 1)))
    feat = e.conv4(h).max(2)[0]
    coarse = d.fc3(F.relu(d.fc2(F.relu(d.fc1(feat))))).view(B, 3, d.num_coarse)
    center = coarse.repeat_interleave(d.scale, dim=2)
    grid = d.grid.unsqueeze(0).repeat(B, 1, d.num_coarse)
    h = torch.cat((grid, center, feat.unsqueeze(2).expand(-1, -1, d.num_fine)), 1)
    fine = d.conv3(F.relu(d.conv2(F.relu(d.conv1(h))))) + center
    return coarse.transpose(1, 2).contiguous(), fine.transpose(1, 2).contiguous()


def _round(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from chamfer3D.model_utils import calc_dcd
    from models.pcn import Model
    if not torch.cuda.is_available():
        raise SystemExit("pcn_bench: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N, NC, NP, W = a.batch, 2048, 1024, 2048, 0.5
    opts = {"alpha": 200, "lambda": 0.5}
    m = Model(types.SimpleNamespace(num_points=NP, loss="dcd", eval_emd=False, loss_opts=opts), num_coarse=NC).to(dev)
    m.decoder.grid = m.decoder.grid.to(dev)
    g = torch.Generator().manual_seed(0)
    gt = (torch.rand(B, NP, 3, generator=g) - 0.5).to(dev)
    x = gt[:, :N].transpose(1, 2).contiguous()

    def hip():
        m.zero_grad(set_to_none=True)
        total = m(x, gt, is_training=True, alpha=W)[2]
        total.backward()
        return total.detach()

    def composed():
        m.zero_grad(set_to_none=True)
        out1, out2 = torch_forward(m, x)
        l1 = calc_dcd(out1, gt, alpha=opts["alpha"], n_lambda=opts["lambda"])[0]
        l2 = calc_dcd(out2, gt, alpha=opts["alpha"], n_lambda=opts["lambda"])[0]
        total = l1.mean() + l2.mean() * W
        total.backward()
        return total.detach()

    fns = {"hip": hip, "torch": composed}
    res = {"iters": a.iters, "rounds": a.rounds, "batch": B}
    tot, grads = {}, {}
    for k, fn in fns.items():
        tot[k] = float(fn())
        grads[k] = [p.grad.clone() for p in m.parameters()]
    res["loss_hip"], res["loss_torch"] = tot["hip"], tot["torch"]
    # the arbiter: the composition with float64 parameters and activations (the loss itself casts to
    # fp32, as calc_dcd does); per version the largest error of a parameter gradient, as a share of
    # that tensor's largest float64 entry
    m64 = copy.deepcopy(m).double()
    m64.decoder.grid = m.decoder.grid.double()
    o1, o2 = torch_forward(m64, x.double())
    (calc_dcd(o1, gt, alpha=opts["alpha"], n_lambda=opts["lambda"])[0].mean()
     + calc_dcd(o2, gt, alpha=opts["alpha"], n_lambda=opts["lambda"])[0].mean() * W).backward()
    names = [k for k, _ in m.named_parameters()]
    for k in fns:
        errs = [float((g.double() - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-300))
                for g, p in zip(grads[k], m64.parameters())]
        res[f"grad_err_vs_float64_{k}"] = {"max": max(errs), "tensor": names[errs.index(max(errs))],
                                           "all": {n: float(f"{e:.3e}") for n, e in zip(names, errs)}}
    del grads, m64, o1, o2
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for k, fn in fns.items():                      # peak memory of one step
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        res[k] = {"peak_mb": (torch.cuda.max_memory_allocated() - base) / 1e6}
    times = {k: [] for k in fns}
    for _ in range(a.rounds):                      # alternate the versions
        for k, fn in fns.items():
            times[k].append(_round(fn, a.iters))
    for k, v in times.items():
        res[k].update({"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)})
    res["torch_over_hip"] = res["torch"]["median_us"] / res["hip"]["median_us"]
    print(f"PCN step B {B}: hip {res['hip']['median_us']:.0f} us ({res['hip']['min_us']:.0f}-{res['hip']['max_us']:.0f}) "
          f"{res['hip']['peak_mb']:.0f} MB  torch {res['torch']['median_us']:.0f} us ({res['torch']['min_us']:.0f}-"
          f"{res['torch']['max_us']:.0f}) {res['torch']['peak_mb']:.0f} MB  torch/hip {res['torch_over_hip']:.2f}  "
          f"loss {tot['hip']:.6f} vs {tot['torch']:.6f}  worst gradient error vs float64: hip "
          f"{res['grad_err_vs_float64_hip']['max']:.2e} ({res['grad_err_vs_float64_hip']['tensor']}), torch "
          f"{res['grad_err_vs_float64_torch']['max']:.2e} ({res['grad_err_vs_float64_torch']['tensor']})", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
