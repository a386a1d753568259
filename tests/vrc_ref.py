"""Restatement of VRCNet's self-attention encoder (Density_aware_Chamfer_Distance/models/vrcnet.py:15-290)
in torch on the CPU, float64 by default, from the contracts of include/ured_hip.h: point-major rows,
gathered tensors built in full. TEST INFRASTRUCTURE ONLY.

Weights and inputs are regenerated from seeds: the make_*_params functions build nn.Conv2d / nn.Linear
layers in the reference's construction order under torch.manual_seed, so they draw the numbers the
reference's own modules draw (tests/golden/make_golden_vrcnet.py asserts this). Every discrete decision
can be forced through a `Dec`: ReLU masks (name -> bool tensor), pool slots, max winners and the
kNN / FPS / pooling-neighbour / three-NN indices; every run records its own decisions with the margin
of each (the distance of the deciding value from a flip).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN_SEED = 7
GRAD_CAP = 128
ENC = dict(B=2, C_in=4, pts_num=[64, 32, 16, 8], k=[4, 8], pk=4, layers=[1, 1, 1, 1], output_size=32)
SA = dict(B=2, N=16, in_planes=32, rel=4, mid=16, out_planes=32, share=8, k=4)
SK = dict(B=2, N=16, in_planes=32, rel=4, mid=16, out_planes=32, share=8, k=[4, 8])
UNIT = dict(B=2, N=16, input_size=6, output_size=32, k=[4, 8], layers=2)
LRB = dict(B=5, input_size=24, output_size=10)
GEO_MARGIN = 1e-4          # every geometric decision of the golden seed is at least this far from a flip


def grad_sub(t):
    """At most GRAD_CAP evenly strided elements of the flattened tensor."""
    flat = t.reshape(-1)
    return flat[::max(1, -(-flat.numel() // GRAD_CAP))]


# ---------------- parameters, in the reference's construction order ----------------

def _sa_layers(p, cin, rel, mid, cout, share, k):
    ms = mid // share
    return [(p + "conv1", nn.Conv2d(cin, rel, 1)), (p + "conv2", nn.Conv2d(cin, rel, 1)), (p + "conv3", nn.Conv2d(cin, mid, 1)),
            (p + "conv_w.1", nn.Conv2d(rel * (k + 1), ms, 1, bias=False)), (p + "conv_w.3", nn.Conv2d(ms, k * ms, 1)),
            (p + "conv_out", nn.Conv2d(mid, cout, 1))]


def _sk_layers(p, cin, rel, mid, cout, share, ks, r=2, L=32):
    d = max(int(cout / r), L)
    out = []
    for i, k in enumerate(ks):
        out += _sa_layers(f"{p}sams.{i}.", cin, rel, mid, cout, share, k)
    out.append((p + "fc", nn.Linear(cout, d)))
    out += [(f"{p}fcs.{i}", nn.Linear(d, cout)) for i in range(len(ks))]
    return out


def _unit_layers(p, cin, cout, ks, layers):
    out = [(p + "conv1", nn.Conv2d(cin, cout, 1, bias=False))]
    for i in range(layers):
        out += _sk_layers(f"{p}sam.{i}.", cout, cout // 16, cout // 4, cout, 8, ks)
    return out + [(p + "conv2", nn.Conv2d(cout, cout, 1, bias=False)), (p + "conv_res", nn.Conv2d(cin, cout, 1, bias=False))]


def _encoder_layers(cin, ks, output_size, layers):
    c1, c2, c3, c4 = 64, 128, 256, 512
    out = _unit_layers("sam_res1.", cin, c1, ks, layers[0]) + _unit_layers("sam_res2.", c2, c2, ks, layers[1])
    out += _unit_layers("sam_res3.", c3, c3, ks, layers[2]) + _unit_layers("sam_res4.", c4, c4, ks, layers[3])
    out += [("conv5", nn.Conv2d(c4, 1024, 1)), ("fc1", nn.Linear(1024, 512)), ("fc2", nn.Linear(512, 1024)),
            ("conv6", nn.Conv2d(c4 + 1024, c4, 1)), ("conv7", nn.Conv2d(c3 + c4, c3, 1)), ("conv8", nn.Conv2d(c2 + c3, c2, 1)),
            ("conv9", nn.Conv2d(c1 + c2, c1, 1)), ("conv_out", nn.Conv2d(c1, output_size, 1))]
    return out


def _state(layers):
    sd = {}
    for n, m in layers:
        sd[n + ".weight"] = m.weight.detach().clone()
        if m.bias is not None:
            sd[n + ".bias"] = m.bias.detach().clone()
    return sd


def make_sa_params(seed, cin, rel, mid, cout, share, k):
    torch.manual_seed(seed)
    return _state(_sa_layers("", cin, rel, mid, cout, share, k))


def make_sk_params(seed, cin, rel, mid, cout, share, ks):
    torch.manual_seed(seed)
    return _state(_sk_layers("", cin, rel, mid, cout, share, ks))


def make_unit_params(seed, cin, cout, ks, layers):
    torch.manual_seed(seed)
    return _state(_unit_layers("", cin, cout, ks, layers))


def make_encoder_params(seed, cin, ks, output_size, layers):
    torch.manual_seed(seed)
    return _state(_encoder_layers(cin, ks, output_size, layers))


def make_lrb_params(seed, input_size, output_size):
    torch.manual_seed(seed)
    return _state([("conv1", nn.Linear(input_size, input_size)), ("conv2", nn.Linear(input_size, output_size)),
                   ("conv_res", nn.Linear(input_size, output_size))])


def make_points(seed, B, N):
    """[B, N, 3] float32, uniform in [-1, 1]^3."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, N, 3, generator=g) * 2 - 1


def make_features(seed, B, C, N, scale=1.0):
    r = np.random.Generator(np.random.PCG64(100 + seed))
    return torch.from_numpy(r.standard_normal((B, C, N)).astype(np.float32) * np.float32(scale))


def make_encoder_input(seed, B, C_in, N):
    """[B, C_in, N]: the coordinates, then C_in - 3 feature channels."""
    x = make_points(seed, B, N).transpose(1, 2)
    return x if C_in == 3 else torch.cat((x, make_features(seed, B, C_in - 3, N)), 1)


def cotangent(seed, shape):
    r = np.random.Generator(np.random.PCG64(1000 + seed))
    return torch.from_numpy(r.standard_normal(shape))


# ---------------- decisions ----------------

class Dec:
    """Forced decisions in, recorded decisions and margins out."""

    def __init__(self, force=None):
        self.force = force or {}
        self.pre, self.mask = {}, {}            # ReLU layers: pre-activation, mask used
        self.idx, self.margin = {}, {}          # discrete picks by name, and their margins

    def relu(self, name, y):
        self.pre[name] = y.detach()
        m = self.force[name] if name in self.force else (y > 0)
        self.mask[name] = m
        return y * m.to(y.dtype)

    def pick(self, name, fn):
        """fn() -> (indices, margin); a forced pick skips the margin."""
        if name in self.force:
            self.idx[name] = self.force[name]
            return self.force[name]
        i, mg = fn()
        self.idx[name], self.margin[name] = i, mg
        return i

    def masks(self):
        return dict(self.mask)


def _d2(a, b):
    """Direct squared distances [B, M, N] of a [B, M, D] to b [B, N, D], summed over ascending d."""
    out = torch.zeros(a.shape[0], a.shape[1], b.shape[1], dtype=a.dtype)
    for d in range(a.shape[2]):
        df = a[:, :, None, d] - b[:, None, :, d]
        out = out + df * df
    return out


def knn_pick(q, p, k):
    """The k points of p nearest to each q by (distance, index) -> (idx [B, M, k], the smallest gap
    between consecutive ranks among the first k + 1)."""
    d = _d2(q, p)
    kk = min(k + 1, p.shape[1])
    order = torch.argsort(d, dim=2, stable=True)[:, :, :kk]
    ds = torch.gather(d, 2, order)
    gap = (ds[:, :, 1:] - ds[:, :, :-1]).min().item() if kk > 1 else float("inf")
    return order[:, :, :k], gap


def fps_pick(p, S):
    """Farthest-point sampling from index 0 on the direct squared distance, lowest index on a tie ->
    (idx [B, S], the smallest winner-to-runner-up gap)."""
    B, N, _ = p.shape
    idx = torch.zeros(B, S, dtype=torch.long)
    best = torch.full((B, N), float("inf"), dtype=p.dtype)
    gap = float("inf")
    last = torch.zeros(B, dtype=torch.long)
    for s in range(1, S):
        c = p[torch.arange(B), last]
        best = torch.minimum(best, _d2(p, c[:, None, :]).squeeze(2))
        last = best.argmax(1)                     # torch.argmax returns the first maximal index
        if N > 1:
            top = best.topk(2, dim=1)[0]
            gap = min(gap, (top[:, 0] - top[:, 1]).min().item())
        idx[:, s] = last
    return idx, gap


# ---------------- kernels' contracts ----------------

def gather_rows(x, idx):
    """x [B, N, C], idx [B, M, k] -> [B, M, k, C]; an index outside [0, N) reads as a zero row."""
    B, N, C = x.shape
    ok = (idx >= 0) & (idx < N)
    safe = idx.clamp(0, N - 1).long()
    g = x[torch.arange(B).view(B, 1, 1), safe]
    return g * ok.unsqueeze(-1).to(x.dtype)


def sa_core(P, idx, Wa, Wb, bb, rel, mid, share, dec, tag="sa"):
    """SaFn's contract. P [B*N, 2 rel + mid], idx [B, N, k] -> o [B*N, mid]."""
    B, N, k = idx.shape
    ms = mid // share
    Pm = dec.relu(tag + ".P", P[:, :2 * rel]).view(B, N, 2 * rel)
    x1, x2 = Pm[:, :, :rel], Pm[:, :, rel:]
    v = gather_rows(x2, idx).permute(0, 1, 3, 2).reshape(B, N, rel * k)          # r k + j
    u = torch.cat((x1, v), 2)
    h = dec.relu(tag + ".h", (u @ Wa.t()).view(B * N, ms))
    w = (h @ Wb.t() + bb).view(B, N, ms, k)
    x3 = gather_rows(P[:, 2 * rel:].view(B, N, mid), idx)                        # [B, N, k, mid]
    wf = w.repeat(1, 1, share, 1)                                                # channel c uses w[c mod ms]
    return dec.relu(tag + ".o", (wf * x3.permute(0, 1, 3, 2)).sum(3).view(B * N, mid))


def _w2(w):
    return w.reshape(w.shape[0], -1)


def sa_module(Pr, p, x, idx, dec, tag="sa"):
    """x [B*N, C] -> [B*N, out]."""
    rel, mid = Pr[p + "conv1.weight"].shape[0], Pr[p + "conv3.weight"].shape[0]
    ms = Pr[p + "conv_w.1.weight"].shape[0]
    W = torch.cat((_w2(Pr[p + "conv1.weight"]), _w2(Pr[p + "conv2.weight"]), _w2(Pr[p + "conv3.weight"])), 0)
    b = torch.cat((Pr[p + "conv1.bias"], Pr[p + "conv2.bias"], Pr[p + "conv3.bias"]), 0)
    P = dec.relu(tag + ".x", x) @ W.t() + b
    o = sa_core(P, idx, _w2(Pr[p + "conv_w.1.weight"]), _w2(Pr[p + "conv_w.3.weight"]), Pr[p + "conv_w.3.bias"], rel, mid,
                mid // ms, dec, tag)
    return o @ _w2(Pr[p + "conv_out.weight"]).t() + Pr[p + "conv_out.bias"] + x


def sk_mean(ys, B):
    U = sum(F.relu(y) for y in ys)
    return U.view(B, -1, U.shape[1]).mean(1)


def sk_mix(a, ys, B, relu_out=False, mask=None):
    """mask: the trailing ReLU's decisions, forced."""
    C = ys[0].shape[1]
    v = sum(a[:, i].unsqueeze(1) * F.relu(y).view(B, -1, C) for i, y in enumerate(ys)).reshape(-1, C)
    if not relu_out:
        return v
    return F.relu(v) if mask is None else v * mask.to(v.dtype)


def sk_sa_module(Pr, p, x, idxs, B, dec, relu_out=False, tag="sk"):
    ys = [sa_module(Pr, f"{p}sams.{i}.", x, idx, dec, f"{tag}.sam{i}") for i, idx in enumerate(idxs)]
    C = ys[0].shape[1]
    fs = [dec.relu(f"{tag}.fea{i}", y) for i, y in enumerate(ys)]
    s = sum(fs).view(B, -1, C).mean(1)
    z = F.linear(s, Pr[p + "fc.weight"], Pr[p + "fc.bias"])
    a = torch.softmax(torch.stack([F.linear(z, Pr[f"{p}fcs.{i}.weight"], Pr[f"{p}fcs.{i}.bias"]) for i in range(len(ys))], 1), 1)
    v = sum(a[:, i].unsqueeze(1) * f.view(B, -1, C) for i, f in enumerate(fs)).reshape(-1, C)
    return dec.relu(tag + ".v", v) if relu_out else v


def skn_res_unit(Pr, p, feat, idxs, B, dec, tag="unit"):
    x = feat @ _w2(Pr[p + "conv1.weight"]).t()
    n = 0
    while f"{p}sam.{n}.fc.weight" in Pr:
        n += 1
    for i in range(n):
        x = sk_sa_module(Pr, f"{p}sam.{i}.", x, idxs, B, dec, i == n - 1, f"{tag}.sk{i}")
    if n == 0:
        x = dec.relu(tag + ".x", x)
    return x @ _w2(Pr[p + "conv2.weight"]).t() + feat @ _w2(Pr[p + "conv_res.weight"]).t()


def linear_resblock(Pr, x, dec):
    """Linear_ResBlock: the reference's ReLU is in place, so conv_res reads the rectified input as well."""
    f = dec.relu("lrb.x", x)
    h = dec.relu("lrb.h", F.linear(f, Pr["conv1.weight"], Pr["conv1.bias"]))
    return F.linear(h, Pr["conv2.weight"], Pr["conv2.bias"]) + F.linear(f, Pr["conv_res.weight"], Pr["conv_res.bias"])


def edge_pool(feat, p_idx, pn_idx, dec, name="slot"):
    """feat [B, N, C] -> (rows [B*S, 2C], slot [B, S, C]); the lowest j wins a tie."""
    B, N, C = feat.shape
    S = p_idx.shape[1]
    centre = gather_rows(feat, p_idx.unsqueeze(2)).squeeze(2)
    nb = gather_rows(feat, pn_idx)                                               # [B, S, pk, C]

    def own():
        sl = _first_max(nb, 2)
        if nb.shape[2] > 1:
            top = nb.topk(2, dim=2)[0]
            return sl, (top[:, :, 0] - top[:, :, 1])
        return sl, torch.full(sl.shape, float("inf"))
    sl = dec.pick(name, own).long()
    best = nb.gather(2, sl.unsqueeze(2)).squeeze(2)
    return torch.cat((centre, best), 2).view(B * S, 2 * C), sl


def _first_max(t, dim):
    """The lowest index of the maximum along dim."""
    mx = t.max(dim, keepdim=True)[0]
    n = t.shape[dim]
    shape = [1] * t.dim()
    shape[dim] = n
    j = torch.arange(n).view(shape).expand_as(t)
    return torch.where(t == mx, j, torch.full_like(j, n)).min(dim)[0]


def three_nn_weights(tgt, src, idx):
    """weight = (1 / dist) / sum(1 / dist), dist = max(sqrt(d^2), 1e-10), for given idx [B, N, K]."""
    d2 = torch.gather(_d2(tgt, src), 2, idx.long())
    inv = 1.0 / torch.sqrt(d2).clamp(min=1e-10)
    return inv / inv.sum(2, keepdim=True)


def unpool(feat2, idx, weight, skip):
    """feat2 [B, S, D2], idx / weight [B, N, K], skip [B, N, D1] | None -> [B*N, D2 + D1], interpolation first."""
    B, N, _ = idx.shape
    out = (gather_rows(feat2, idx) * weight.unsqueeze(-1)).sum(2)
    if skip is not None:
        out = torch.cat((out, skip), 2)
    return out.reshape(B * N, -1)


def encoder(Pr, features, cfg, dec):
    """features [B, C_in, N] -> [B, output_size, N]. The geometry runs in features' dtype unless forced."""
    B, _, N = features.shape
    ks, pk, pts_num = cfg["k"], cfg["pk"], cfg["pts_num"]
    pts = [features[:, 0:3, :].detach().transpose(1, 2).contiguous()]
    x = features.transpose(1, 2).reshape(B * N, -1)
    skips = []
    for lv in range(4):
        if lv:
            src = pts[-1]
            p_idx = dec.pick(f"fps{lv}", lambda: fps_pick(src, pts_num[lv]))
            out_pts = torch.gather(src, 1, p_idx.long().unsqueeze(-1).expand(-1, -1, 3))
            pn_idx = dec.pick(f"pn_idx{lv}", lambda: knn_pick(out_pts, src, min(pk, src.shape[1])))
            x, _ = edge_pool(skips[-1].view(B, src.shape[1], -1), p_idx, pn_idx, dec, f"slot{lv}")
            pts.append(out_pts)
        cur = pts[lv]
        idxs = [dec.pick(f"knn{lv + 1}.{i}", lambda k=k: knn_pick(cur, cur, k)) for i, k in enumerate(ks)]
        x = skn_res_unit(Pr, f"sam_res{lv + 1}.", x, idxs, B, dec, f"res{lv + 1}")
        skips.append(dec.relu(f"x{lv + 1}", x))
    x1, x2, x3, x4 = skips
    n4 = pts_num[3]
    y5 = (x4 @ _w2(Pr["conv5.weight"]).t() + Pr["conv5.bias"]).view(B, n4, -1)

    def own():
        top = y5.topk(2, dim=1)[0] if n4 > 1 else None
        return _first_max(y5, 1), (top[:, 0] - top[:, 1]) if top is not None else torch.full((B, y5.shape[2]), float("inf"))
    dec.pre["conv5"] = y5.detach()
    win = dec.pick("win", own).long()
    g = y5.gather(1, win.unsqueeze(1)).squeeze(1)
    g = dec.relu("fc1", F.linear(g, Pr["fc1.weight"], Pr["fc1.bias"]))
    g = dec.relu("fc2", F.linear(g, Pr["fc2.weight"], Pr["fc2.bias"]))
    h = torch.cat((g.unsqueeze(1).expand(-1, n4, -1).reshape(B * n4, -1), x4), 1)
    y = h @ _w2(Pr["conv6.weight"]).t() + Pr["conv6.bias"]
    prev = "conv6"
    for name, lv, skip in (("conv7", 2, x3), ("conv8", 1, x2), ("conv9", 0, x1)):
        tgt, src = pts[lv], pts[lv + 1]
        idx = dec.pick(f"three_nn{lv}", lambda: knn_pick(tgt, src, min(3, src.shape[1])))
        w = three_nn_weights(tgt, src, idx).to(y.dtype)
        u = unpool(dec.relu(prev, y).view(B, src.shape[1], -1), idx, w, skip.view(B, tgt.shape[1], -1))
        y = u @ _w2(Pr[name + ".weight"]).t() + Pr[name + ".bias"]
        prev = name
    out = dec.relu("conv9", y) @ _w2(Pr["conv_out.weight"]).t() + Pr["conv_out.bias"]
    return out.view(B, N, -1).transpose(1, 2)


def run(fn, Pr, inputs, cot=None, dtype=torch.float64, force=None):
    """fn(Pd, *inputs, dec) -> output. Parameters and floating inputs are cast to dtype; returns dict out,
    dec (the Dec of the run), grads (name -> gradient under cot; inputs as 'in0', 'in1', ..)."""
    Pd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in Pr.items()}
    ins = [t.detach().to(dtype).requires_grad_(True) if torch.is_tensor(t) and t.is_floating_point() else t for t in inputs]
    dec = Dec(force)
    out = fn(Pd, *ins, dec)
    res = {"out": out.detach(), "dec": dec, "grads": {}}
    if cot is not None:
        names = list(Pd)
        leaves = [Pd[k] for k in names]
        for i, t in enumerate(ins):
            if torch.is_tensor(t) and t.is_floating_point():
                names.append(f"in{i}")
                leaves.append(t)
        got = torch.autograd.grad((out * cot.to(dtype)).sum(), leaves, allow_unused=True)
        res["grads"] = {n: (torch.zeros_like(l) if g is None else g) for n, l, g in zip(names, leaves, got)}
    return res


# ---------------- the golden fixtures ----------------

def to_rows(x):
    """[B, C, 1, N] or [B, C, N] -> [B*N, C]."""
    if x.dim() == 4:
        x = x.squeeze(2)
    return x.transpose(1, 2).reshape(-1, x.shape[1])


def from_rows(y, B, four=True):
    y = y.view(B, -1, y.shape[1]).transpose(1, 2)
    return y.unsqueeze(2) if four else y


def fixture(name, seed=GOLDEN_SEED):
    """-> (params, x in the reference's layout, idxs (int64, from float64 geometry), cotangent)."""
    if name == "enc":
        E = ENC
        Pr = make_encoder_params(seed, E["C_in"], E["k"], E["output_size"], E["layers"])
        x = make_encoder_input(seed, E["B"], E["C_in"], E["pts_num"][0])
        return Pr, x, None, cotangent(seed, (E["B"], E["output_size"], E["pts_num"][0]))
    if name == "lrb":
        L = LRB
        x = make_features(seed, L["B"], L["input_size"], 1).squeeze(2)          # standard normal: half the entries negative
        return make_lrb_params(seed, L["input_size"], L["output_size"]), x, None, cotangent(seed, (L["B"], L["output_size"]))
    S = {"sa": SA, "sk": SK, "unit": UNIT}[name]
    pts = make_points(seed, S["B"], S["N"]).double()
    ks = S["k"] if isinstance(S["k"], list) else [S["k"]]
    idxs = [knn_pick(pts, pts, k)[0] for k in ks]
    if name == "unit":
        Pr = make_unit_params(seed, S["input_size"], S["output_size"], S["k"], S["layers"])
        cin, cout = S["input_size"], S["output_size"]
    else:
        make = make_sa_params if name == "sa" else make_sk_params
        Pr = make(seed, S["in_planes"], S["rel"], S["mid"], S["out_planes"], S["share"], S["k"])
        cin, cout = S["in_planes"], S["out_planes"]
    x = make_features(seed, S["B"], cin, S["N"]).unsqueeze(2)
    return Pr, x, idxs, cotangent(seed, (S["B"], cout, 1, S["N"]))


def run_fixture(name, dtype=torch.float64, force=None, seed=GOLDEN_SEED):
    """The restatement on a golden fixture, in and out in the reference's layout (grads['in0'] too)."""
    Pr, x, idxs, cot = fixture(name, seed)
    B = x.shape[0]
    if name == "enc":
        return run(lambda P, xx, dec: encoder(P, xx, ENC, dec), Pr, [x], cot, dtype, force)
    if name == "lrb":
        return run(linear_resblock, Pr, [x], cot, dtype, force)
    fn = {"sa": lambda P, xx, dec: from_rows(sa_module(P, "", to_rows(xx), idxs[0], dec), B),
          "sk": lambda P, xx, dec: from_rows(sk_sa_module(P, "", to_rows(xx), idxs, B, dec), B),
          "unit": lambda P, xx, dec: from_rows(skn_res_unit(P, "", to_rows(xx), idxs, B, dec), B)}[name]
    return run(fn, Pr, [x], cot, dtype, force)
