"""Micro-benchmark of the Vector-Neuron kernels (ured_hip.vn, network/VN/) against the torch
composition a user had before them, on the same GPU in the same run.

  python tools/vn_bench.py [--iters 5] [--rounds 7] [--out FILE.json] [--timeout 240]

Shapes are the encoder's own at B 16, N 1024, k 20. Legs: the feature-space kNN in 63 dimensions; one
edge layer (conv3: 21 -> 42) forward + backward with mean and with max pooling; conv5 (170 -> 341,
shared direction) forward + backward; the whole vn_encoder forward + backward with mean pooling. The
baselines, written out below: the [B, N, N] matrix -|a|^2 - |b|^2 + 2ab with topk; the gathered
[B, N, k, 3, 2C] graph feature, two linear maps on it, the norm, BatchNorm on the norms, the
directional leaky ReLU and the pool, all kept by autograd; for the encoder those pieces with the
module's own parameters.

Each leg runs in a child process of its own under a time limit (a leg that fails or runs out of
time ends the run; nothing further is started on the device); at most 16 CPU threads. Per leg both
versions are warmed up, then timed in alternating rounds of `iters` calls between two device
events; the figure is the median round (min and max beside it). Peak memory is the
torch.cuda.max_memory_allocated delta of one call of each version over what is allocated before
it. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, KNN = 16, 1024, 20
LEGS = ["kNN 16x1024 D=63 k=20", "edge layer fwd+bwd 21->42 mean", "edge layer fwd+bwd 21->42 max",
        "conv5 fwd+bwd 170->341", "vn_encoder fwd+bwd 16x1024 mean"]
EPS = 1e-6


# ---------------- the torch baselines (point-major [B, N, 3, C] in and out) ----------------

def knn_torch(x, k):
    import torch
    inner = torch.bmm(x, x.transpose(1, 2))
    sq = (x * x).sum(-1)
    return (2 * inner - sq.unsqueeze(1) - sq.unsqueeze(2)).topk(k, dim=-1)[1]


def vn_act_torch(e, Wf, Wd, bn):
    """e [..., 3, Cin] -> [..., 3, Co]: two linear maps, BatchNorm of the norms, directional leaky ReLU."""
    import torch
    p, d = e @ Wf.t(), e @ Wd.t()
    nrm = torch.norm(p, dim=-2) + EPS
    flat = nrm.reshape(-1, nrm.shape[-1])
    nb = (bn(flat) if isinstance(bn, torch.nn.BatchNorm1d) else bn(flat.view(flat.shape[0], -1, 1, 1))).view(nrm.shape)
    p = p / nrm.unsqueeze(-2) * nb.unsqueeze(-2)
    dot = (p * d).sum(-2, keepdim=True)
    mask = (dot >= 0).float()
    dsq = (d * d).sum(-2, keepdim=True)
    return 0.2 * p + 0.8 * (mask * p + (1 - mask) * (p - (dot / (dsq + EPS)) * d))


def edge_torch(x, idx, layer, pool):
    import torch
    b = torch.arange(x.shape[0], device=x.device).view(-1, 1, 1)
    nb = x[b, idx]                                           # [B, N, k, 3, C]
    ctr = x.unsqueeze(2).expand_as(nb)
    y = vn_act_torch(torch.cat((nb - ctr, ctr), -1), layer.map_to_feat.weight, layer.map_to_dir.weight, layer.batchnorm.bn)
    if pool is None:
        return y.mean(2)
    d = y @ pool.map_to_dir.weight.t()
    win = (y * d).sum(-2).max(dim=2)[1]                      # [B, N, C]
    return torch.gather(y, 2, win.view(win.shape[0], win.shape[1], 1, 1, -1).expand(-1, -1, 1, 3, -1)).squeeze(2)


def point_torch(x, layer):
    return vn_act_torch(x, layer.map_to_feat.weight, layer.map_to_dir.weight, layer.batchnorm.bn)


def encoder_torch(net, pts):
    import torch
    import torch.nn.functional as F
    Bn, _, Nn = pts.shape
    feat = pts.transpose(1, 2).reshape(Bn, Nn, 3, 1)
    levels = []
    for conv in (net.conv1, net.conv2, net.conv3, net.conv4):
        feat = edge_torch(feat, knn_torch(feat.detach().reshape(Bn, Nn, -1), net.n_knn), conv, None)
        levels.append(feat)
    y = point_torch(torch.cat(levels, -1), net.conv5)
    y = torch.cat((y, y.mean(1, keepdim=True).expand_as(y)), -1)
    z = point_torch(point_torch(y, net.std_feature.vn1), net.std_feature.vn2) @ net.std_feature.vn_lin.weight.t()
    flat = torch.einsum("bnjc,bnjk->bnck", y, z).reshape(Bn, Nn, -1)
    pf = net.per_point_f(flat)
    v = torch.cat((flat.max(1)[0], flat.mean(1)), 1)
    return net.linear2(F.leaky_relu(net.bn1(net.linear1(v)), 0.2)), pf.permute(0, 2, 1)


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


def run_leg(leg, iters, rounds):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.add_pkg_path()
    from network.VN import vn_layers as L
    from network.VN.vn_encoder import vn_encoder
    from ured_hip import vn as V
    if not torch.cuda.is_available():
        raise SystemExit("vn_bench: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {}
    i = LEGS.index(leg)

    def stepper(leaves, go):
        def step(fwd):
            for t in leaves:
                t.grad = None
            fwd().backward(go)
        return step

    if i == 0:
        x = torch.randn(B, N, 63, generator=g).to(dev)
        a, b = V.knn_rows(x, KNN).long(), knn_torch(x, KNN)
        res["rows_with_other_neighbour_sets"] = int((a.sort(-1)[0] != b.sort(-1)[0]).any(-1).sum())   # the baseline uses the expansion
        res["rows"] = B * N
        fns = {"hip": lambda: V.knn_rows(x, KNN), "torch": lambda: knn_torch(x, KNN)}
    elif i in (1, 2):
        C, Co = 21, 42
        x = torch.randn(B, N, 3, C, generator=g).to(dev).requires_grad_(True)
        idx = V.knn_rows(x.detach().view(B, N, 3 * C), KNN)
        layer = L.VNLinearLeakyReLU(2 * C, Co).to(dev)
        pool = L.VNMaxPool(Co).to(dev) if i == 2 else None
        go = torch.randn(B, N, 3, Co, generator=g).to(dev)
        step = stepper(list(layer.parameters()) + [x], go)
        il = idx.long()
        if pool is None:
            hip = lambda: layer.forward_graph(x, idx, "mean")                      # noqa: E731
        else:
            hip = lambda: pool.forward_rows(layer.forward_graph(x, idx, "none"))   # noqa: E731
        with torch.no_grad():
            res["max_abs_diff"] = float((hip() - edge_torch(x, il, layer, pool)).abs().max())
        fns = {"hip": lambda: step(hip), "torch": lambda: step(lambda: edge_torch(x, il, layer, pool))}
    elif i == 3:
        C, Co = 170, 341
        x = torch.randn(B, N, 3, C, generator=g).to(dev).requires_grad_(True)
        layer = L.VNLinearLeakyReLU(C, Co, dim=4, share_nonlinearity=True).to(dev)
        go = torch.randn(B, N, 3, Co, generator=g).to(dev)
        step = stepper(list(layer.parameters()) + [x], go)
        with torch.no_grad():
            res["max_abs_diff"] = float((layer.forward_rows(x) - point_torch(x, layer)).abs().max())
        fns = {"hip": lambda: step(lambda: layer.forward_rows(x)), "torch": lambda: step(lambda: point_torch(x, layer))}
    else:
        net = vn_encoder(dict(n_knn=KNN, pooling="mean", target_latent_dim=256)).to(dev).train()
        pts = (torch.rand(B, 3, N, generator=g) * 2 - 1).to(dev)

        def run(fwd):
            for t in net.parameters():
                t.grad = None
            gf, pf = fwd()
            (gf.sum() + pf.sum()).backward()
        fns = {"hip": lambda: run(lambda: net(pts)), "torch": lambda: run(lambda: encoder_torch(net, pts))}
    res.update(measure(fns, iters, rounds))
    res["torch_over_hip"] = res["torch"]["median_us"] / res["hip"]["median_us"]
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
            raise SystemExit(f"vn_bench: leg '{leg}' failed (exit {r.returncode})\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
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
