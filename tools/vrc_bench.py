"""Micro-benchmark of VRCNet's self-attention encoder (ured_hip.vrc, models/vrcnet.py) against the torch
composition of the reference's formulas, on the same GPU in the same run. The encoder leg also counts
the first level's rows whose neighbour set differs between the two versions' searches.

  python tools/vrc_bench.py [--batch 32] [--iters 3] [--rounds 5] [--out FILE.json] [--timeout 300]

Shapes are those of cfgs/vrc_dcd.yaml: N 3072, k 16, pk 10, layers 1,1,1,1, 4 input channels, 32 clouds.
Legs: one SA unit at the first level (C 64: rel 4, mid 16) forward + backward; one edge pool
(3072 -> 1536 points, C 64) forward + backward; one unpool (1536 -> 3072 points, 128 interpolated + 64
skip channels) forward + backward; the whole encoder forward + backward; and, at the shape of cfgs/vrc.yaml
(2048 input points, num_coarse_raw 1024, num_fps 2048, num_coarse 1024, folding, points_label): Folding +
conv_f1 / conv_f2 (1024 -> 2048 points) forward + backward against the [B, G + C + 2, N r] tensor built in
full, and the whole decoder forward + backward; and, at the shape of cfgs/vrc_dcd.yaml (num_coarse == num_fine, KLD,
dcd), one training forward + backward of Model on `batch` pairs, so 2 x batch decoder clouds, against the same
torch encoder / decoder composition with the PCN encoder, the heads, softplus / rsample / kl_divergence and the
loss tail (dense distance matrix, min, visit counts, four heads as the reference calls them) in torch. The baselines, written out
below: the gathered [B, C, k, N] tensor with conv2 / conv3 run on it, the attention weights repeated
over share_planes, all kept by autograd; the gathered [B, C, S, pk] tensor and its max; three gathered
rows times their weights; for the encoder those pieces with the module's own parameters, the
[B, N, N] matrix -|a|^2 - |b|^2 + 2ab with topk for every neighbour search, and the project's FPS kernel
in both versions (torch has none).

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
N, KNN, PK, CIN = 3072, 16, 10, 4
PTS = [3072, 1536, 768, 384]
LEGS = ["SA unit fwd+bwd C64 k16", "edge pool fwd+bwd 3072->1536 C64 pk10", "unpool fwd+bwd 1536->3072 128+64",
        "encoder fwd+bwd", "Folding + conv_f1/f2 fwd+bwd 1024->2048", "decoder fwd+bwd", "model fwd+bwd vrc_dcd"]
# the model leg: cfgs/vrc_dcd.yaml (2048 input and gt points, num_coarse == num_fine: fine is the coarse cloud; KLD, dcd 40 / 0.5)
MODEL = dict(n=2048, n_gt=2048, num_coarse_raw=1024, num_fps=2048, num_coarse=2048, num_points=2048, size_z=128, alpha=0.5,
             t_alpha=40, n_lambda=0.5)
# the decoder legs: cfgs/vrc.yaml (2048 input points, num_coarse_raw 1024, num_fps 2048, num_coarse 1024, folding, points_label)
DEC = dict(n=2048, num_coarse_raw=1024, num_fps=2048, num_coarse=1024, num_fine=2048)


# ---------------- the torch baselines (the reference's layouts: [B, C, 1, N]) ----------------

def gather_torch(x, idx):
    """x [B, C, N], idx [B, M, k] -> [B, C, k, M]."""
    Bn, C, _ = x.shape
    _, M, k = idx.shape
    flat = idx.reshape(Bn, 1, M * k).expand(-1, C, -1)
    return x.gather(2, flat).view(Bn, C, M, k).permute(0, 1, 3, 2)


def knn_torch(q, p, k):
    """q [B, M, 3], p [B, N, 3] -> the k nearest p of every q by the expansion, [B, M, k]."""
    import torch
    inner = torch.bmm(q, p.transpose(1, 2))
    return (2 * inner - (q * q).sum(-1).unsqueeze(2) - (p * p).sum(-1).unsqueeze(1)).topk(k, dim=-1)[1]


def sa_torch(m, x, idx):
    import torch
    import torch.nn.functional as F
    Bn, _, _, Nn = x.shape
    xr = F.relu(x)
    xn = gather_torch(xr.squeeze(2), idx)
    x1 = F.conv2d(xr, m.conv1.weight, m.conv1.bias)
    x2 = F.conv2d(xn, m.conv2.weight, m.conv2.bias).reshape(Bn, -1, 1, Nn)
    x3 = F.conv2d(xn, m.conv3.weight, m.conv3.bias)
    w = m.conv_w(torch.cat((x1, x2), 1)).view(Bn, -1, m.k, Nn).repeat(1, m.share_planes, 1, 1)
    out = F.relu((w * x3).sum(2, keepdim=True))
    return F.conv2d(out, m.conv_out.weight, m.conv_out.bias) + x


def sk_torch(sk, x, idxs):
    import torch
    import torch.nn.functional as F
    feas = torch.stack([F.relu(sa_torch(sam, x, idxs[i])) for i, sam in enumerate(sk.sams)], 1)
    z = sk.fc(feas.sum(1).mean(-1).mean(-1))
    a = torch.softmax(torch.stack([fc(z) for fc in sk.fcs], 1), 1)
    return (feas * a.unsqueeze(-1).unsqueeze(-1)).sum(1)


def unit_torch(u, feat, idxs):
    import torch.nn.functional as F
    x = F.conv2d(feat, u.conv1.weight)
    for sk in u.sam:
        x = sk_torch(sk, x, idxs)
    return F.conv2d(F.relu(x), u.conv2.weight) + F.conv2d(feat, u.conv_res.weight)


def pool_torch(feat, p_idx, pn_idx):
    """feat [B, C, N] -> [B, 2C, S]."""
    import torch
    centre = feat.gather(2, p_idx.unsqueeze(1).expand(-1, feat.shape[1], -1))
    return torch.cat((centre, gather_torch(feat, pn_idx).max(2)[0]), 1)


def unpool_torch(feat2, idx, weight, skip):
    """feat2 [B, D2, S], idx / weight [B, N, 3], skip [B, D1, N] -> [B, D2 + D1, N]."""
    import torch
    return torch.cat(((gather_torch(feat2, idx) * weight.transpose(1, 2).unsqueeze(1)).sum(2), skip), 1)


def encoder_torch(net, feats):
    import torch
    import torch.nn.functional as F
    from ured_hip import group
    Bn = feats.shape[0]
    pts = [feats[:, 0:3, :].detach().transpose(1, 2).contiguous()]
    x = feats.unsqueeze(2)
    skips = []
    for lv, unit in enumerate((net.sam_res1, net.sam_res2, net.sam_res3, net.sam_res4)):
        if lv:
            src = pts[-1]
            p_idx = group.fps(src, net.pts_num[lv], start=torch.zeros(Bn, dtype=torch.int32, device=src.device)).long()
            out_pts = src.gather(1, p_idx.unsqueeze(-1).expand(-1, -1, 3))
            x = pool_torch(skips[-1].squeeze(2), p_idx, knn_torch(out_pts, src, net.pk)).unsqueeze(2)
            pts.append(out_pts)
        x = unit_torch(unit, x, [knn_torch(pts[lv], pts[lv], k) for k in net.k])
        skips.append(F.relu(x))
    x1, x2, x3, x4 = skips
    g = F.conv2d(x4, net.conv5.weight, net.conv5.bias).max(-1)[0].view(Bn, -1)
    g = net.dropout(F.relu(net.fc2(net.dropout(F.relu(net.fc1(g))))))
    y = F.conv2d(torch.cat((g.view(Bn, -1, 1, 1).expand(-1, -1, 1, net.pts_num[3]), x4), 1), net.conv6.weight, net.conv6.bias)
    for conv, lv, skip in ((net.conv7, 2, x3), (net.conv8, 1, x2), (net.conv9, 0, x1)):
        d, idx = torch.cdist(pts[lv], pts[lv + 1]).topk(3, dim=-1, largest=False)
        inv = 1.0 / d.clamp(min=1e-10)
        u = unpool_torch(F.relu(y).squeeze(2), idx, inv / inv.sum(2, keepdim=True), skip.squeeze(2)).unsqueeze(2)
        y = F.conv2d(u, conv.weight, conv.bias)
    return F.conv2d(F.relu(y), net.conv_out.weight, net.conv_out.bias).squeeze(2)


def folding_torch(m, point_feat, global_feat):
    """Folding on the [B, G + C + 2, N r] tensor built in full. point_feat [B, C, N], global_feat [B, G]."""
    import torch
    import torch.nn.functional as F
    Bn, _, Nn = point_feat.shape
    r = m.step_ratio
    feats = torch.cat((global_feat.unsqueeze(2).expand(-1, -1, Nn * r), point_feat.repeat_interleave(r, dim=2),
                       m.grid.t().repeat(1, Nn).unsqueeze(0).expand(Bn, -1, -1)), 1)
    return F.relu(F.conv1d(feats, m.conv.weight, m.conv.bias))


def fold_tail_torch(dec, feat, g):
    """expansion2 (Folding) + conv_f1 + conv_f2 -> [B, 3, N r]."""
    import torch.nn.functional as F
    up = folding_torch(dec.expansion2, feat, g)
    return F.conv1d(F.relu(F.conv1d(up, dec.conv_f1.weight, dec.conv_f1.bias)), dec.conv_f2.weight, dec.conv_f2.bias)


def fold_tail_hip(dec, rows, g):
    """The same layers as the decoder runs them: rows [B*N, C] -> [B*N*r, 3]."""
    from ured_hip.vrc import linear_rows
    up = dec.expansion2.forward_rows(rows, g)
    f1 = linear_rows(up, dec.conv_f1.weight.squeeze(2), dec.conv_f1.bias)
    return linear_rows(f1, dec.conv_f2.weight.squeeze(2), dec.conv_f2.bias, relu_in=True)


def decoder_torch(net, g, pin):
    """The folding / points_label decoder without an expansion1, in torch: encoder_torch, topk for the ranking,
    torch.gather, the project's FPS kernel (torch has none)."""
    import torch
    import torch.nn.functional as F
    from ured_hip import group
    Bn = g.shape[0]
    raw = net.fc3(F.relu(net.fc2(F.relu(net.fc1(g))))).view(Bn, 3, -1)
    pts = torch.cat((torch.cat((raw, raw.new_zeros(Bn, 1, raw.shape[2])), 1), torch.cat((pin, pin.new_ones(Bn, 1, pin.shape[2])), 1)), 2)
    feat = F.relu(F.conv1d(encoder_torch(net.encoder, pts), net.conv_cup1.weight, net.conv_cup1.bias))
    high = F.conv1d(feat, net.conv_cup2.weight, net.conv_cup2.bias)

    def take(t, idx):
        return t.gather(2, idx.unsqueeze(1).expand(-1, t.shape[1], -1))
    cur = high
    if cur.shape[2] > net.num_fps:
        idx = group.fps(high.detach().transpose(1, 2).contiguous(), net.num_fps,
                        start=torch.zeros(Bn, dtype=torch.int32, device=g.device)).long()
        cur, feat = take(cur, idx), take(feat, idx)
    if cur.shape[2] > net.num_coarse:
        sc = F.softplus(net.conv_s3(F.relu(net.conv_s2(F.relu(net.conv_s1(feat))))))
        idx = sc.topk(net.num_coarse, dim=2)[1].view(Bn, -1)
        cur, feat = take(cur, idx), take(feat, idx)
    if cur.shape[2] >= net.num_fine:                  # num_coarse == num_fine: the coarse cloud is the output
        return raw, high, cur, cur
    fine = fold_tail_torch(net, feat, g) + cur.repeat_interleave(net.expansion2.step_ratio, dim=2)
    return raw, high, cur, fine


def pcn_encoder_torch(e, x):
    import torch
    import torch.nn.functional as F
    y2 = F.conv1d(F.relu(F.conv1d(x, e.conv1.weight, e.conv1.bias)), e.conv2.weight, e.conv2.bias)
    h = torch.cat((y2, y2.max(2, keepdim=True)[0].expand(-1, -1, x.shape[2])), 1)
    return F.conv1d(F.relu(F.conv1d(h, e.conv3.weight, e.conv3.bias)), e.conv4.weight, e.conv4.bias).max(2)[0]


def lrb_torch(m, f):
    import torch.nn.functional as F
    f = F.relu(f)
    return m.conv2(F.relu(m.conv1(f))) + m.conv_res(f)


def dcd_torch(x, gt, alpha, n_lambda):
    """calc_dcd's formulas on the dense [B, n_gt, n_x] matrix of squared distances -> the per-cloud loss."""
    import torch
    d = torch.cdist(gt, x) ** 2
    (dist1, idx1), (dist2, idx2) = d.min(2), d.min(1)
    n_x, n_gt = x.shape[1], gt.shape[1]
    cnt1 = torch.zeros_like(idx2).scatter_add_(1, idx1, torch.ones_like(idx1))
    cnt2 = torch.zeros_like(idx1).scatter_add_(1, idx2, torch.ones_like(idx2))
    w1 = (cnt1.gather(1, idx1).float() ** n_lambda + 1e-6) ** (-1) * (n_gt / n_x)
    w2 = (cnt2.gather(1, idx2).float() ** n_lambda + 1e-6) ** (-1) * (n_x / n_gt)
    return ((1 - torch.exp(-dist1 * alpha) * w1).mean(1) + (1 - torch.exp(-dist2 * alpha) * w2).mean(1)) / 2


def model_torch(net, x, gt, alpha, eps_q, eps_p):
    """Model's training forward (KLD, dcd) in torch, the reference's four heads; the project's FPS kernel picks y."""
    import torch
    import torch.nn.functional as F
    from torch.distributions import Normal, kl_divergence
    from ured_hip import group
    Bn, Z = x.shape[0], net.size_z
    idx = group.fps(gt, x.shape[2], start=torch.zeros(Bn, dtype=torch.int32, device=gt.device)).long()
    y = gt.gather(1, idx.unsqueeze(-1).expand(-1, -1, 3)).transpose(1, 2)
    feat = pcn_encoder_torch(net.encoder, torch.cat((x, y), 0))
    fx = F.relu(feat[:Bn])
    o_x = lrb_torch(net.posterior_infer2, lrb_torch(net.posterior_infer1, fx))
    o_y = lrb_torch(net.prior_infer, feat[Bn:])
    q = Normal(o_x[:, :Z], F.softplus(o_x[:, Z:]))
    p = Normal(o_y[:, :Z], F.softplus(o_y[:, Z:]))
    z = torch.cat((q.loc + q.scale * eps_q, p.loc + p.scale * eps_p), 0)
    dl_rec = kl_divergence(Normal(torch.zeros_like(p.loc), torch.ones_like(p.scale)), p)
    dl_g = kl_divergence(Normal(p.loc.detach(), p.scale.detach()), q)
    code = torch.cat((fx, fx), 0) + lrb_torch(net.generator, z)
    clouds = [c.transpose(1, 2).contiguous() for c in decoder_torch(net.decoder, code, torch.cat((x, x), 0))]
    gt2 = torch.cat((gt, gt), 0)
    ta, nl = net.loss_opts["alpha"], net.loss_opts["lambda"]
    l = [dcd_torch(c, gt2, ta * 2 if i == 0 else ta, nl) for i, c in enumerate(clouds)]
    return l[0].mean() * 10 + l[1].mean() * 0.5 + l[2].mean() + l[3].mean() * alpha + (dl_rec.mean() + dl_g.mean()) * 20


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


def measure(fns, iters, rounds, warm=2):
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


def run_leg(leg, B, iters, rounds):
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.add_pkg_path()
    from chamfer3D.model_utils import knn, three_nn_upsampling
    from models import vrcnet as M
    from ured_hip import vrc as V
    if not torch.cuda.is_available():
        raise SystemExit("vrc_bench: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"batch": B}
    i = LEGS.index(leg)
    pts = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)

    def stepper(leaves, go):
        def step(fwd):
            for t in leaves:
                t.grad = None
            fwd().backward(go)
        return step

    if i == 0:
        C = 64
        mod = M.SA_module(C, C // 16, C // 4, C, 8, KNN).to(dev)
        x = torch.randn(B, C, 1, N, generator=g).to(dev).requires_grad_(True)
        idx = knn(pts.transpose(1, 2), KNN)
        go = torch.randn(B, C, 1, N, generator=g).to(dev)
        step = stepper(list(mod.parameters()) + [x], go)
        with torch.no_grad():
            res["max_abs_diff"] = float((mod([x, idx])[0] - sa_torch(mod, x, idx)).abs().max())
        fns = {"hip": lambda: step(lambda: mod([x, idx])[0]), "torch": lambda: step(lambda: sa_torch(mod, x, idx))}
    elif i == 1:
        from ured_hip import group
        C, S = 64, PTS[1]
        feat = torch.randn(B, N, C, generator=g).to(dev).requires_grad_(True)
        p_idx = group.fps(pts, S, start=torch.zeros(B, dtype=torch.int32, device=dev))
        pn_idx = knn_torch(pts.gather(1, p_idx.long().unsqueeze(-1).expand(-1, -1, 3)), pts, PK).int()
        go = torch.randn(B * S, 2 * C, generator=g).to(dev)
        pl, nl = p_idx.long(), pn_idx.long()

        def base():
            return pool_torch(feat.transpose(1, 2), pl, nl).transpose(1, 2).reshape(B * S, 2 * C)
        with torch.no_grad():
            res["max_abs_diff"] = float((V.EdgePoolFn.apply(feat, p_idx, pn_idx)[0] - base()).abs().max())
        step = stepper([feat], go)
        fns = {"hip": lambda: step(lambda: V.EdgePoolFn.apply(feat, p_idx, pn_idx)[0]), "torch": lambda: step(base)}
    elif i == 2:
        S, D2, D1 = PTS[1], 128, 64
        src = pts[:, :S].contiguous()
        feat2 = torch.randn(B, S, D2, generator=g).to(dev).requires_grad_(True)
        skip = torch.randn(B, N, D1, generator=g).to(dev).requires_grad_(True)
        idx, w = three_nn_upsampling(pts, src)
        il = idx.long()
        go = torch.randn(B * N, D2 + D1, generator=g).to(dev)

        def base():
            return unpool_torch(feat2.transpose(1, 2), il, w, skip.transpose(1, 2)).transpose(1, 2).reshape(B * N, D2 + D1)
        with torch.no_grad():
            res["max_abs_diff"] = float((V.UnpoolFn.apply(feat2, idx, w, skip) - base()).abs().max())
        step = stepper([feat2, skip], go)
        fns = {"hip": lambda: step(lambda: V.UnpoolFn.apply(feat2, idx, w, skip)), "torch": lambda: step(base)}
    elif i == 4:
        net = M.MSAP_SKN_decoder(DEC["num_coarse_raw"], DEC["num_fps"], DEC["num_coarse"], DEC["num_fine"], [1, 1, 1, 1], [KNN], PK,
                                 points_label=True, local_folding=True).to(dev).eval()
        nc = DEC["num_coarse"]
        feat = torch.randn(B, 64, nc, generator=g).to(dev).requires_grad_(True)
        gf = torch.randn(B, 1024, generator=g).to(dev).requires_grad_(True)
        go = torch.randn(B, 3, DEC["num_fine"], generator=g).to(dev)
        leaves = [feat, gf] + [p for m in (net.expansion2, net.conv_f1, net.conv_f2) for p in m.parameters()]
        step = stepper(leaves, go)

        def hip():
            return fold_tail_hip(net, feat.transpose(1, 2).reshape(B * nc, 64), gf).view(B, DEC["num_fine"], 3).transpose(1, 2)
        with torch.no_grad():
            res["max_abs_diff"] = float((hip() - fold_tail_torch(net, feat, gf)).abs().max())
        fns = {"hip": lambda: step(hip), "torch": lambda: step(lambda: fold_tail_torch(net, feat, gf))}
    elif i == 5:
        net = M.MSAP_SKN_decoder(DEC["num_coarse_raw"], DEC["num_fps"], DEC["num_coarse"], DEC["num_fine"], [1, 1, 1, 1], [KNN], PK,
                                 points_label=True, local_folding=True).to(dev).eval()
        gf = torch.randn(B, 1024, generator=g).to(dev).requires_grad_(True)
        pin = (torch.rand(B, 3, DEC["n"], generator=g) * 2 - 1).to(dev).requires_grad_(True)
        leaves = list(net.parameters()) + [gf, pin]
        gos = None

        def step(fwd):
            for t in leaves:
                t.grad = None
            outs = fwd()
            torch.autograd.backward(outs, gos)
        with torch.no_grad():
            a, b = net(gf, pin), decoder_torch(net, gf, pin)
            gos = [torch.randn(o.shape, generator=g).to(dev) for o in a]
            res["max_abs_diff"] = float((a[0] - b[0]).abs().max())              # coarse_raw: before any search or selection
            res["coarse_high_max_abs_diff"] = float((a[1] - b[1]).abs().max())  # after the encoder's two kNN versions
        fns = {"hip": lambda: step(lambda: net(gf, pin)), "torch": lambda: step(lambda: decoder_torch(net, gf, pin))}
    elif i == 6:
        import types
        Mo = MODEL
        args = types.SimpleNamespace(layers="1,1,1,1", knn_list=str(KNN), distribution_loss="KLD", loss="dcd",
                                     loss_opts={"alpha": Mo["t_alpha"], "lambda": Mo["n_lambda"]}, eval_emd=False,
                                     num_fps=Mo["num_fps"], num_points=Mo["num_points"], num_coarse=Mo["num_coarse"],
                                     num_coarse_raw=Mo["num_coarse_raw"], pk=PK, local_folding=True, points_label=True)
        net = M.Model(args, size_z=Mo["size_z"]).to(dev).eval()
        x = (torch.rand(B, 3, Mo["n"], generator=g) * 2 - 1).to(dev)
        gt = (torch.rand(B, Mo["n_gt"], 3, generator=g) * 2 - 1).to(dev)
        eps = [torch.randn(B, Mo["size_z"], generator=g).to(dev) for _ in range(2)]
        leaves = [q for q in net.parameters()]

        def step(fwd):
            for t in leaves:
                t.grad = None
            fwd().backward()
        with torch.no_grad():
            a, b = net(x, gt, alpha=Mo["alpha"], noise=eps)[2], model_torch(net, x, gt, Mo["alpha"], *eps)
            res["total_hip"], res["total_torch"] = float(a), float(b)
            res["max_abs_diff"] = abs(float(a) - float(b))       # of the two totals (the two kNN versions differ in a few rows)
        res["decoder_clouds"] = 2 * B
        fns = {"hip": lambda: step(lambda: net(x, gt, alpha=Mo["alpha"], noise=eps)[2]),
               "torch": lambda: step(lambda: model_torch(net, x, gt, Mo["alpha"], *eps))}
    else:
        net = M.SA_SKN_Res_encoder(CIN, [KNN], PK, 64, [1, 1, 1, 1], PTS).to(dev).eval()
        feats = torch.cat((pts.transpose(1, 2), torch.randn(B, CIN - 3, N, generator=g).to(dev)), 1).requires_grad_(True)
        go = torch.randn(B, 64, N, generator=g).to(dev)
        step = stepper(list(net.parameters()) + [feats], go)
        with torch.no_grad():
            res["max_abs_diff"] = float((net(feats) - encoder_torch(net, feats)).abs().max())
            a, b = knn(pts.transpose(1, 2), KNN), knn_torch(pts, pts, KNN)      # the first level's two searches
            res["level1_rows_with_other_neighbour_sets"] = int((a.sort(-1)[0] != b.sort(-1)[0]).any(-1).sum())
            res["level1_rows"] = B * N
        fns = {"hip": lambda: step(lambda: net(feats)), "torch": lambda: step(lambda: encoder_torch(net, feats))}
    res.update(measure(fns, iters, rounds))
    res["torch_over_hip"] = res["torch"]["median_us"] / res["hip"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--leg", default=None, help="(internal) run this one leg and print its JSON")
    a = ap.parse_args()
    if a.leg is not None:
        print(json.dumps(run_leg(a.leg, a.batch, a.iters, a.rounds)))
        return
    res = {"batch": a.batch, "iters": a.iters, "rounds": a.rounds, "legs": {}}
    for leg in LEGS:      # one child per leg, each under its own time limit; the first failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(a.batch), "--iters",
                            str(a.iters), "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            raise SystemExit(f"vrc_bench: leg '{leg}' failed (exit {r.returncode})\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        v = json.loads(r.stdout.strip().splitlines()[-1])
        res["legs"][leg] = v
        print(f"{leg}: hip {v['hip']['median_us']:.1f} us ({v['hip']['min_us']:.1f}-{v['hip']['max_us']:.1f}) "
              f"{v['hip']['peak_mb']:.1f} MB  torch {v['torch']['median_us']:.1f} us ({v['torch']['min_us']:.1f}-"
              f"{v['torch']['max_us']:.1f}) {v['torch']['peak_mb']:.1f} MB  torch/hip {v['torch_over_hip']:.2f}  "
              f"max |diff| {v['max_abs_diff']:.2e}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
