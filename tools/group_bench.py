"""Micro-benchmark of the set-abstraction kernels (ured_hip.group, network/pointnet/pointnet2_utils)
against the torch composition a user had before them, on the same GPU in the same run.

  python tools/group_bench.py [--iters 10] [--rounds 7] [--out FILE.json] [--timeout 240]

Legs: farthest-point sampling 16x2048 -> 512 and 16x1024 -> 128; ball query 16x2048, S = 512,
r = 0.2, nsample = 32; grouping forward + backward on that shape with D = 64; one set-abstraction
layer (512, 0.2, 32, 3 + 3, [64, 64, 128]) forward + backward; the feature-propagation interpolation
(three neighbours given) forward + backward at 16x2048 from 512, D2 = 256; one feature-propagation
layer (384, [256, 256]) forward + backward on that shape with D1 = 128; one multi-scale layer
(512, [0.1, 0.2, 0.4], [32, 64, 128], 3, [[32, 32, 64], [64, 64, 128], [64, 96, 128]]) forward +
backward. The baselines: a Python loop of
npoint iterations (gather the centroid, distances, masked minimum update, argmax) for the sampling;
the B x S x N distance matrix by |a|^2 + |b|^2 - 2ab, a mask and a sort for the ball query;
advanced indexing and a cat (and their autograd) for the grouping; all of those plus
Conv2d / BatchNorm2d / ReLU / max for the layer; for the interpolation the reciprocal weights,
advanced indexing and weighted sum of the reference's feature propagation on the same neighbours,
for its layer also the B x N x S distance matrix, the full sort, the cat and Conv1d / BatchNorm1d /
ReLU; for the multi-scale layer the set-abstraction baseline once per scale and a cat.

Each leg runs in a child process of its own under a time limit (a leg that fails or runs out of
time ends the run; nothing further is started on the device); at most 16 CPU threads. Per leg both
versions are warmed up, then timed in alternating rounds of `iters` calls between two device
events; the figure is the median round (min and max beside it). The shader clock is noted when the
runtime reports one. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ["fps 16x2048->512", "fps 16x1024->128", "ball query 16x2048 S=512 r=0.2 ns=32",
        "group fwd+bwd 16x2048 S=512 K=32 D=64", "SA layer fwd+bwd (512, 0.2, 32, 3+3, [64,64,128])",
        "interp fwd+bwd 16x2048 from 512 D2=256", "FP layer fwd+bwd (384, [256,256]) 16x2048 from 512",
        "MSG layer fwd+bwd (512, [0.1,0.2,0.4], [32,64,128], 3, 3 scales)"]


# ---------------- the torch baselines ----------------

def fps_torch(xyz, npoint, start):
    import torch
    B, N, _ = xyz.shape
    out = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    dmin = torch.full((B, N), 1e10, device=xyz.device)
    far = start
    rows = torch.arange(B, device=xyz.device)
    for i in range(npoint):
        out[:, i] = far
        c = xyz[rows, far].view(B, 1, 3)
        d = ((xyz - c) ** 2).sum(-1)
        m = d < dmin
        dmin[m] = d[m]
        far = dmin.max(-1)[1]
    return out


def ball_torch(radius, nsample, xyz, new_xyz):
    import torch
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    d = -2 * torch.matmul(new_xyz, xyz.transpose(1, 2))
    d += (new_xyz ** 2).sum(-1).view(B, S, 1)
    d += (xyz ** 2).sum(-1).view(B, 1, N)
    idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat(B, S, 1)
    idx[d > radius ** 2] = N
    idx = idx.sort(dim=-1)[0][:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, nsample)
    pad = idx == N
    idx[pad] = first[pad]
    return idx


def gather_torch(points, idx):
    import torch
    B = points.shape[0]
    b = torch.arange(B, device=points.device).view(B, *([1] * (idx.dim() - 1))).expand_as(idx)
    return points[b, idx]


def group_torch(xyz, new_xyz, points, idx):
    import torch
    B, S, _ = new_xyz.shape
    g = gather_torch(xyz, idx) - new_xyz.view(B, S, 1, 3)
    return torch.cat([g, gather_torch(points, idx)], -1)


def interp_torch(points2, idx, d):
    """The reference's weights, gather and weighted sum (pointnet2_utils.py:300-303) on given neighbours."""
    r = 1.0 / (d + 1e-8)
    w = r / r.sum(dim=2, keepdim=True)
    return (gather_torch(points2, idx) * w.unsqueeze(-1)).sum(dim=2)


def three_nn_torch(xyz1, xyz2):
    import torch
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    d = -2 * torch.matmul(xyz1, xyz2.transpose(1, 2))
    d += (xyz1 ** 2).sum(-1).view(B, N, 1)
    d += (xyz2 ** 2).sum(-1).view(B, 1, S)
    d, idx = d.sort(dim=-1)
    return d[:, :, :3], idx[:, :, :3]


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
    times = {k: [] for k in fns}
    for _ in range(rounds):                        # alternate the versions
        for k, fn in fns.items():
            times[k].append(_round(fn, iters))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


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
    from ured_hip import group as G
    from network.pointnet import pointnet2_utils as P
    if not torch.cuda.is_available():
        raise SystemExit("group_bench: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"clock_mhz_before": _clock()}
    i = LEGS.index(leg)
    if i < 2:
        N, npoint = ((2048, 512), (1024, 128))[i]
        xyz = torch.rand(16, N, 3, generator=g).to(dev)
        start = torch.randint(0, N, (16,), generator=g).to(dev)
        fns = {"hip": lambda: G.fps(xyz, npoint, start), "torch": lambda: fps_torch(xyz, npoint, start)}
        res["same_indices"] = bool((G.fps(xyz, npoint, start).long() == fps_torch(xyz, npoint, start)).all())
    else:
        B, N, S, K, r = 16, 2048, 512, 32, 0.2
        xyz = torch.rand(B, N, 3, generator=g).to(dev)
        start = torch.randint(0, N, (B,), generator=g).to(dev)
        new_xyz = gather_torch(xyz, G.fps(xyz, S, start).long())
        if i == 2:
            fns = {"hip": lambda: G.ball_query(r, K, xyz, new_xyz), "torch": lambda: ball_torch(r, K, xyz, new_xyz)}
            a, b = G.ball_query(r, K, xyz, new_xyz).long(), ball_torch(r, K, xyz, new_xyz)
            res["rows_with_other_indices"] = int((a != b).any(-1).sum())    # the baseline uses the expansion
            res["rows"] = B * S
        elif i == 3:
            pts = torch.randn(B, N, 64, generator=g).to(dev)
            idx = G.ball_query(r, K, xyz, new_xyz)
            idl = idx.long()
            go = torch.randn(B * S * K, 67, generator=g).to(dev)
            leaves = [t.clone().requires_grad_(True) for t in (xyz, new_xyz, pts)]

            def step(fwd):
                for t in leaves:
                    t.grad = None
                fwd(*leaves).reshape(B * S * K, 67).backward(go)

            fns = {"hip": lambda: step(lambda x, c, p: G.GroupFn.apply(x, c, p, idx)),
                   "torch": lambda: step(lambda x, c, p: group_torch(x, c, p, idl))}
        elif i >= 5:
            fns = _fp_msg_legs(i, torch, G, P, dev, g, xyz, new_xyz, start, res)
        else:
            layer = P.PointNetSetAbstraction(S, r, K, 3 + 3, [64, 64, 128], False).to(dev).train()
            feats = torch.randn(B, 3, N, generator=g).to(dev).requires_grad_(True)
            x_bcn = xyz.transpose(1, 2).contiguous()           # first-layer coordinates: no gradient asked
            go = torch.randn(B, 128, S, generator=g).to(dev)
            params = list(layer.parameters())

            def torch_layer(x, f):
                xt, ft = x.permute(0, 2, 1), f.permute(0, 2, 1)
                nx = gather_torch(xt, fps_torch(xt, S, start))
                h = group_torch(xt, nx, ft, ball_torch(r, K, xt, nx)).permute(0, 3, 2, 1)
                for conv, bn in zip(layer.mlp_convs, layer.mlp_bns):
                    h = torch.relu(bn(conv(h)))
                return nx.permute(0, 2, 1), h.max(2)[0]

            def step(fwd):
                for t in params + [feats]:
                    t.grad = None
                fwd(x_bcn, feats)[1].backward(go)

            fns = {"hip": lambda: step(lambda x, f: layer(x, f, start=start)), "torch": lambda: step(torch_layer)}
    res.update(measure(fns, iters, rounds))
    res["torch_over_hip"] = res["torch"]["median_us"] / res["hip"]["median_us"]
    res["clock_mhz_after"] = _clock()
    return res


def _fp_msg_legs(i, torch, G, P, dev, g, xyz, new_xyz, start, res):
    """The feature-propagation and multi-scale legs: xyz [16,2048,3] fine, new_xyz [16,512,3] its sample."""
    from ured_hip import interp as I
    B, N, S = xyz.shape[0], xyz.shape[1], new_xyz.shape[1]
    if i == 5:      # the interpolation alone, on given neighbours
        D2 = 256
        d, idx = I.three_nn(xyz, new_xyz)
        idl = idx.long()
        p2 = torch.randn(B, S, D2, generator=g).to(dev).requires_grad_(True)
        dl = d.detach().clone().requires_grad_(True)
        go = torch.randn(B * N, D2, generator=g).to(dev)
        with torch.no_grad():
            res["max_abs_diff"] = float((I.InterpFn.apply(None, p2, idx, dl).view(B, N, D2) - interp_torch(p2, idl, dl)).abs().max())

        def step(fwd):
            p2.grad = dl.grad = None
            fwd().reshape(B * N, D2).backward(go)

        return {"hip": lambda: step(lambda: I.InterpFn.apply(None, p2, idx, dl)),
                "torch": lambda: step(lambda: interp_torch(p2, idl, dl))}
    if i == 6:      # one feature-propagation layer, coordinates constant (as in a segmentation decoder's use)
        D1, D2 = 128, 256
        layer = P.PointNetFeaturePropagation(D1 + D2, [256, 256]).to(dev).train()
        x1, x2 = xyz.transpose(1, 2).contiguous(), new_xyz.transpose(1, 2).contiguous()
        p1 = torch.randn(B, D1, N, generator=g).to(dev).requires_grad_(True)
        p2 = torch.randn(B, D2, S, generator=g).to(dev).requires_grad_(True)
        go = torch.randn(B, 256, N, generator=g).to(dev)
        leaves = list(layer.parameters()) + [p1, p2]

        def torch_layer():
            d, idx = three_nn_torch(xyz, new_xyz)
            h = torch.cat([p1.permute(0, 2, 1), interp_torch(p2.permute(0, 2, 1), idx, d)], -1).permute(0, 2, 1)
            for conv, bn in zip(layer.mlp_convs, layer.mlp_bns):
                h = torch.relu(bn(conv(h)))
            return h

        def step(fwd):
            for t in leaves:
                t.grad = None
            fwd().backward(go)

        return {"hip": lambda: step(lambda: layer(x1, x2, p1, p2)), "torch": lambda: step(torch_layer)}
    radii, ns, mlps = [0.1, 0.2, 0.4], [32, 64, 128], [[32, 32, 64], [64, 64, 128], [64, 96, 128]]
    layer = P.PointNetSetAbstractionMsg(S, radii, ns, 3, mlps).to(dev).train()
    feats = torch.randn(B, 3, N, generator=g).to(dev).requires_grad_(True)
    x_bcn = xyz.transpose(1, 2).contiguous()
    go = torch.randn(B, 64 + 128 + 128, S, generator=g).to(dev)
    leaves = list(layer.parameters()) + [feats]

    def torch_layer():
        ft = feats.permute(0, 2, 1)
        nx = gather_torch(xyz, fps_torch(xyz, S, start))
        outs = []
        for radius, k, convs, bns in zip(radii, ns, layer.conv_blocks, layer.bn_blocks):
            idx = ball_torch(radius, k, xyz, nx)
            h = torch.cat([gather_torch(ft, idx), gather_torch(xyz, idx) - nx.view(B, S, 1, 3)], -1).permute(0, 3, 2, 1)
            for conv, bn in zip(convs, bns):
                h = torch.relu(bn(conv(h)))
            outs.append(h.max(2)[0])
        return torch.cat(outs, 1)

    def step(fwd):
        for t in leaves:
            t.grad = None
        fwd().backward(go)

    return {"hip": lambda: step(lambda: layer(x_bcn, feats, start=start)[1]), "torch": lambda: step(torch_layer)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
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
            raise SystemExit(f"group_bench: leg '{leg}' failed (exit {r.returncode})\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        v = json.loads(r.stdout.strip().splitlines()[-1])
        res["legs"][leg] = v
        print(f"{leg}: hip {v['hip']['median_us']:.1f} us ({v['hip']['min_us']:.1f}-{v['hip']['max_us']:.1f})  "
              f"torch {v['torch']['median_us']:.1f} us ({v['torch']['min_us']:.1f}-{v['torch']['max_us']:.1f})  "
              f"torch/hip {v['torch_over_hip']:.2f}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
