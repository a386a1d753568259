"""Micro-benchmark of the 3D-GCN kernels (ured_hip.gcn, network/P_3DGC.py, network/gc3d_encoder.py)
against the torch composition a user had before them, on the same GPU in the same run.

  python tools/gcn_bench.py [--iters 5] [--rounds 7] [--out FILE.json] [--timeout 240]

Shapes are the encoder's own: B 16, V 2048 / 512 / 128, n 10 neighbours, S 7 supports, C 128 / 256.
Legs: the neighbour search (n + 1 nearest, first dropped); the unit directions; Conv_surface,
Conv_layer (128 -> 128 at V 2048, 256 -> 256 at V 512 and V 128) and Pool_layer forward + backward;
the whole GCN3D_ENCODER forward + backward at 16 x 2048. The baselines, written out below: the
[B, V, V] matrix |a|^2 + |b|^2 - 2ab with topk for the search; advanced indexing, a subtraction and
F.normalize for the directions; for the layers the [B, V, n, S*C] tensors theta = relu(directions @
supports), the gathered support features and their product, a max over n and a sum over S, all
kept by autograd; for the pooling the gather and max of every vertex followed by the sample; for the
encoder those pieces with nn.BatchNorm1d and nn.Conv1d, on the same parameters and the same samples.

Each leg runs in a child process of its own under a time limit (a leg that fails or runs out of
time ends the run; nothing further is started on the device); at most 16 CPU threads. Per leg both
versions are warmed up, then timed in alternating rounds of `iters` calls between two device
events; the figure is the median round (min and max beside it). Peak memory is the
torch.cuda.max_memory_allocated delta of one call of each version over what is allocated before
it. The shader clock is noted when the runtime reports one. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N_NUM, SUP = 16, 10, 7
LEGS = ["neighbour index 16x2048 n=10", "directions 16x2048 n=10", "Conv_surface fwd+bwd 16x2048 C=128",
        "Conv_layer fwd+bwd 16x2048 128->128", "Conv_layer fwd+bwd 16x512 256->256",
        "Conv_layer fwd+bwd 16x128 256->256", "Pool_layer fwd+bwd 16x2048 C=128",
        "GCN3D_ENCODER fwd+bwd 16x2048"]


# ---------------- the torch baselines ----------------

def neighbours_torch(v, n):
    import torch
    sq = (v * v).sum(-1)
    d = sq.unsqueeze(1) + sq.unsqueeze(2) - 2 * torch.bmm(v, v.transpose(1, 2))
    return d.topk(n + 1, dim=-1, largest=False)[1][:, :, 1:]


def nearest_torch(a, b):
    import torch
    d = (b * b).sum(-1).unsqueeze(1) + (a * a).sum(-1).unsqueeze(2) - 2 * torch.bmm(a, b.transpose(1, 2))
    return d.topk(1, dim=-1, largest=False)[1]


def gather_torch(t, idx):
    import torch
    b = torch.arange(t.shape[0], device=t.device).view(-1, 1, 1)
    return t[b, idx]


def dirs_torch(v, idx):
    import torch.nn.functional as F
    return F.normalize(gather_torch(v, idx) - v.unsqueeze(2), dim=-1)


def surface_torch(directions, S, idx, v):
    import torch
    import torch.nn.functional as F
    bs, V, n = idx.shape
    theta = torch.relu(dirs_torch(v, idx) @ F.normalize(directions, dim=0))
    return theta.view(bs, V, n, S, -1).max(2)[0].sum(2)


def layer_torch(weights, bias, directions, S, idx, v, fm):
    import torch
    import torch.nn.functional as F
    bs, V, n = idx.shape
    C = directions.shape[1] // S
    theta = torch.relu(dirs_torch(v, idx) @ F.normalize(directions, dim=0))
    out = fm @ weights + bias
    act = (theta * gather_torch(out[:, :, C:], idx)).view(bs, V, n, S, C)
    return out[:, :, :C] + act.max(2)[0].sum(2)


def pool_torch(v, fm, sample, k=4):
    pooled = gather_torch(fm, neighbours_torch(v, k)).max(2)[0]
    return v[:, sample], pooled[:, sample]


def encoder_torch(net, v, samples):
    import torch

    def layer(m, idx, vv, fm):
        return layer_torch(m.weights, m.bias, m.directions, m.support_num, idx, vv, fm)

    def bn_relu(bn, fm):
        return torch.relu(bn(fm.transpose(1, 2)).transpose(1, 2))

    idx = neighbours_torch(v, net.neighbor_num)
    fm_0 = torch.relu(surface_torch(net.conv_0.directions, net.support_num, idx, v))
    fm_1 = bn_relu(net.bn1, layer(net.conv_1, idx, v, fm_0))
    v1, fp1 = pool_torch(v, fm_1, samples[0])
    idx = neighbours_torch(v1, min(net.neighbor_num, v1.shape[1] // 8))
    fm_2 = bn_relu(net.bn2, layer(net.conv_2, idx, v1, fp1))
    fm_3 = bn_relu(net.bn3, layer(net.conv_3, idx, v1, fm_2))
    v2, fp2 = pool_torch(v1, fm_3, samples[1])
    idx = neighbours_torch(v2, min(net.neighbor_num, v2.shape[1] // 8))
    fm_4 = layer(net.conv_4, idx, v2, fp2)
    n1, n2 = nearest_torch(v, v1), nearest_torch(v, v2)
    cat = torch.cat([fm_0, fm_1, gather_torch(fm_2, n1).squeeze(2), gather_torch(fm_3, n1).squeeze(2),
                     gather_torch(fm_4, n2).squeeze(2)], dim=2)
    return fm_4.max(1)[0], net.conv1d_block(cat.permute(0, 2, 1))


# ---------------- timing ----------------

def _round(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def measure(fns, iters, rounds, warm=3):
    import torch
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {}
    for k, fn in fns.items():                      # peak memory of one call
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        out[k] = {"peak_mb": (torch.cuda.max_memory_allocated() - base) / 1e6}
    times = {k: [] for k in fns}
    for _ in range(rounds):                        # alternate the versions
        for k, fn in fns.items():
            times[k].append(_round(fn, iters))
    for k, v in times.items():
        out[k].update({"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)})
    return out


def _clock():
    import torch
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def run_leg(leg, iters, rounds):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.add_pkg_path()
    import network.P_3DGC as M
    from network.gc3d_encoder import GCN3D_ENCODER
    if not torch.cuda.is_available():
        raise SystemExit("gcn_bench: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"clock_mhz_before": _clock()}
    i = LEGS.index(leg)
    V = {4: 512, 5: 128}.get(i, 2048)
    v = torch.rand(B, V, 3, generator=g).to(dev)
    idx = M.get_neighbor_index(v, N_NUM)

    def stepper(leaves, go):
        def step(fwd):
            for t in leaves:
                t.grad = None
            fwd().backward(go)
        return step

    if i == 0:
        fns = {"hip": lambda: M.get_neighbor_index(v, N_NUM), "torch": lambda: neighbours_torch(v, N_NUM)}
        res["entries_with_other_indices"] = int((idx != neighbours_torch(v, N_NUM)).sum())   # the baseline uses the expansion
        res["entries"] = idx.numel()
    elif i == 1:
        fns = {"hip": lambda: M.get_neighbor_direction_norm(v, idx), "torch": lambda: dirs_torch(v, idx)}
        res["max_abs_diff"] = float((M.get_neighbor_direction_norm(v, idx) - dirs_torch(v, idx)).abs().max())
    elif i == 2:
        mod = M.Conv_surface(128, SUP).to(dev)
        go = torch.randn(B, V, 128, generator=g).to(dev)
        step = stepper(list(mod.parameters()), go)
        fns = {"hip": lambda: step(lambda: mod(idx, v)),
               "torch": lambda: step(lambda: surface_torch(mod.directions, SUP, idx, v))}
    elif i in (3, 4, 5):
        C = 128 if i == 3 else 256
        mod = M.Conv_layer(C, C, SUP).to(dev)
        fm = torch.randn(B, V, C, generator=g).to(dev).requires_grad_(True)
        go = torch.randn(B, V, C, generator=g).to(dev)
        step = stepper(list(mod.parameters()) + [fm], go)
        with torch.no_grad():
            d = mod(idx, v, fm) - layer_torch(mod.weights, mod.bias, mod.directions, SUP, idx, v, fm)
            res["max_abs_diff"] = float(d.abs().max())
        fns = {"hip": lambda: step(lambda: mod(idx, v, fm)),
               "torch": lambda: step(lambda: layer_torch(mod.weights, mod.bias, mod.directions, SUP, idx, v, fm))}
    elif i == 6:
        mod = M.Pool_layer(4, 4)
        fm = torch.randn(B, V, 128, generator=g).to(dev).requires_grad_(True)
        go = torch.randn(B, V // 4, 128, generator=g).to(dev)
        step = stepper([fm], go)
        sample = torch.randperm(V)[:V // 4].to(dev)
        fns = {"hip": lambda: step(lambda: mod(v, fm)[1]), "torch": lambda: step(lambda: pool_torch(v, fm, sample)[1])}
    else:
        net = GCN3D_ENCODER().to(dev).train()
        def total(out):
            return out[1].sum() + out[0].sum()

        def hip():
            torch.manual_seed(1)
            for t in net.parameters():
                t.grad = None
            total(net(v)).backward()

        def plain():
            torch.manual_seed(1)
            samples = (torch.randperm(V)[:V // 4].to(dev), torch.randperm(V // 4)[:V // 16].to(dev))
            for t in net.parameters():
                t.grad = None
            total(encoder_torch(net, v, samples)).backward()

        fns = {"hip": hip, "torch": plain}
    res.update(measure(fns, iters, rounds))
    res["torch_over_hip"] = res["torch"]["median_us"] / res["hip"]["median_us"]
    res["clock_mhz_after"] = _clock()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    ap.add_argument("--leg", default=None, help="(internal) run this one leg and print its JSON")
    a = ap.parse_args()
    if a.leg is not None:
        print(json.dumps(run_leg(a.leg, a.iters, a.rounds)))
        return
    res = {"iters": a.iters, "rounds": a.rounds, "legs": {}}
    for leg in LEGS:      # one child per leg, each under its own time limit; the first failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--iters", str(a.iters), "--rounds",
                            str(a.rounds)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            raise SystemExit(f"gcn_bench: leg '{leg}' failed (exit {r.returncode})\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        v = json.loads(r.stdout.strip().splitlines()[-1])
        res["legs"][leg] = v
        print(f"{leg}: hip {v['hip']['median_us']:.1f} us ({v['hip']['min_us']:.1f}-{v['hip']['max_us']:.1f}) "
              f"{v['hip']['peak_mb']:.1f} MB  torch {v['torch']['median_us']:.1f} us ({v['torch']['min_us']:.1f}-"
              f"{v['torch']['max_us']:.1f}) {v['torch']['peak_mb']:.1f} MB  torch/hip {v['torch_over_hip']:.2f}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
