"""Plain-torch restatement of the three fused MLP chains of ured_hip/mlp.py — TEST INFRASTRUCTURE.

One function per autograd Function, point-major like the Functions, autograd for the backward:

  encoder_ref   PointEncoderFn   7 x (Conv -> BN -> ReLU) with the semantics joined at layer 6,
                                 max-pool of layer 6 over each group + fc, per-point head
  residual_ref  ResidualNetFn    cat(pp, code[group]) -> 3 x (Conv -> ReLU -> BN) -> Conv
  chain_ref     PointChainFn     L x (Conv -> BN (-> ReLU)), max-pool and / or last activation

Each takes the Function's parameter list (32, 14 or 4L tensors in the Function's order, any
widths; conv weights [N, K] or [N, K, 1]) and returns a Ref: the outputs and, per BN layer, the raw
Y, the batch mean / invstd / scale / shift, z (Y * scale + shift for Conv->BN(->ReLU) layers, the
normalised relu(Y) for Conv->ReLU->BN layers), the ReLU mask, the updated running statistics, and
the pool winners (point within group, ties to the lowest point). Ref.grads(...) runs the backward.

decisions = {"masks": [bool [M, N] or None per layer], "winners": int [G, N] or None}: ReLU masks
applied instead of the layer's own `> 0` (the ReLU is always h = z * mask, so autograd routes the
gradient by the mask that was used) and pool winners gathered instead of the argmax. With them a
float64 run follows the discrete choices an fp32 implementation made; Ref.decisions() returns a
run's own.

row_weights [G] (with fixed group_rows): the call is a unique-row batch, group g standing for
w[g] identical groups. The expanded batch is what is evaluated; outputs, Y, z and masks are
reported for the stored rows (the first copy of each group), and an output gradient handed to
grads() is the sum over the copies' gradients, as the unique-row caller passes it (BN's backward
only sees that sum, so it is placed on the first copy). Parameter gradients are those of the
expanded batch, input gradients are summed over the copies.
"""
import torch

ACT_ENC, ACT_RES, ACT_BN = 0, 1, 2       # ured_hip.kernels.ACT_*
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


class Ref:
    """Result of one reference run. outputs: tuple (None for an output not asked for); layers:
    list of dicts per BN layer; winners: [G, N] or None; inputs / params: the leaves."""

    def __init__(self, outputs, layers, winners, inputs, params):
        self.outputs, self.layers, self.winners = outputs, layers, winners
        self.inputs, self.params = inputs, params

    def decisions(self):
        return {"masks": [L["mask"] for L in self.layers], "winners": self.winners}

    def grads(self, *gout):
        """Backward from output gradients (None: that output is unused). Returns ({input name:
        gradient or None}, [parameter gradient or None])."""
        outs, gs = [], []
        for o, g in zip(self.outputs, gout):
            if o is not None and g is not None:
                outs.append(o)
                gs.append(g.detach().cpu().to(o.dtype))
        names = [k for k, v in self.inputs.items() if v.requires_grad]
        leaves = [self.inputs[k] for k in names] + list(self.params)
        got = torch.autograd.grad(outs, leaves, gs, allow_unused=True, retain_graph=True)
        gin = {k: None for k in self.inputs}
        gin.update(dict(zip(names, got[:len(names)])))
        return gin, list(got[len(names):])


def _leaf(t, dtype, grad=True):
    t = t.detach().cpu().to(dtype).clone()
    return t.requires_grad_(grad and t.numel() > 0)


def _w2(W):
    return W.reshape(W.shape[0], -1)


def _running(running, i, N, dtype):
    if running is None:
        return torch.zeros(N, dtype=dtype), torch.ones(N, dtype=dtype), 0
    rm, rv, nbt = running[i]
    return rm.detach().cpu().to(dtype), rv.detach().cpu().to(dtype), int(nbt)


class _Rows:
    """Row bookkeeping of a (possibly unique-row) batch of G groups of group_rows rows."""

    def __init__(self, M, group_rows, row_weights):
        self.M, self.GR = M, group_rows
        self.G = M // group_rows if group_rows else 0
        self.weighted = row_weights is not None
        if not self.weighted:
            self.groups = torch.arange(self.G)              # stored group of each evaluated group
            self.rows = None                                # evaluated row -> stored row
            self.first_g = self.groups
            self.first = None
            return
        w = [int(v) for v in row_weights.detach().cpu().tolist()]
        assert len(w) == self.G and all(v >= 1 for v in w) and all(float(a) == float(b) for a, b in
                                                                   zip(w, row_weights.detach().cpu().tolist()))
        self.groups = torch.repeat_interleave(torch.arange(self.G), torch.tensor(w))
        ar = torch.arange(group_rows)
        self.rows = (self.groups.unsqueeze(1) * group_rows + ar).reshape(-1)
        starts = torch.cumsum(torch.tensor([0] + w[:-1]), 0)
        self.first_g = starts                               # first copy of each stored group
        self.first = (starts.unsqueeze(1) * group_rows + ar).reshape(-1)

    def expand(self, t):        # stored rows -> evaluated rows
        return t if self.rows is None else t[self.rows]

    def expand_groups(self, t):
        return t if not self.weighted else t[self.groups]

    def stored(self, t):        # evaluated rows -> stored rows (first copies)
        return t if self.first is None else t[self.first]

    def stored_groups(self, t):
        return t if not self.weighted else t[self.first_g]


def _bn_layer(Y, act, gamma, beta, run, training, eps, momentum, mask, rows):
    """One BN layer on the evaluated batch. Returns (h, record)."""
    rm, rv, nbt = run
    if act == ACT_RES:
        m = (Y > 0) if mask is None else rows.expand(mask.detach().cpu().bool())
        v = Y * m.to(Y.dtype)
    else:
        v = Y
    if training:
        n = v.shape[0]
        mean = v.mean(0)
        var = ((v - mean) ** 2).mean(0)
        invstd = torch.rsqrt(var + eps)
        new_rm = (1 - momentum) * rm + momentum * mean.detach()
        new_rv = (1 - momentum) * rv + momentum * var.detach() * (n / max(n - 1, 1))
        nbt += 1
    else:
        mean, invstd = rm, torch.rsqrt(rv + eps)
        new_rm, new_rv = rm, rv
    scale = gamma * invstd
    shift = beta - mean * scale
    z = v * scale + shift
    if act == ACT_ENC:
        m = (z > 0) if mask is None else rows.expand(mask.detach().cpu().bool())
        h = z * m.to(z.dtype)
    else:
        h = z
    rec = dict(Y=rows.stored(Y), z=rows.stored(z), mask=None if act == ACT_BN else rows.stored(m).detach(),
               mean=mean, invstd=invstd, scale=scale, shift=shift, act=act,
               running_mean=new_rm, running_var=new_rv, num_batches_tracked=nbt)
    return h, rec


def _pool(h, rows, winners):
    """Max over each evaluated group of h [Me, N] -> (pooled [Ge, N], stored winners [G, N])."""
    N = h.shape[1]
    hg = h.view(-1, rows.GR, N)
    if winners is None:
        mx = hg.detach().amax(dim=1, keepdim=True)
        ar = torch.arange(rows.GR).view(1, -1, 1)
        idx = torch.where(hg.detach() == mx, ar, rows.GR).amin(dim=1)        # lowest point among the maxima
    else:
        idx = rows.expand_groups(winners.detach().cpu().long())
    pooled = hg.gather(1, idx.unsqueeze(1)).squeeze(1)
    return pooled, rows.stored_groups(idx)


def _masks(decisions, n):
    if decisions is None or decisions.get("masks") is None:
        return [None] * n
    assert len(decisions["masks"]) == n
    return decisions["masks"]


def _winners(decisions):
    return None if decisions is None else decisions.get("winners")


def encoder_ref(params, x, sem, mode, group_rows, *, training=True, eps=BN_EPS, momentum=BN_MOMENTUM,
                running=None, decisions=None, row_weights=None, dtype=torch.float64):
    """PointEncoderFn: x [M, 3 (any Cin)], sem [G, S] (mode "src") or [M, S] ("tgt"). Outputs
    (code [G, C], pp [M, C])."""
    assert mode in ("src", "tgt") and len(params) == 32
    P = [_leaf(p, dtype) for p in params]
    xl, seml = _leaf(x, dtype), _leaf(sem, dtype)
    rows = _Rows(xl.shape[0], group_rows, row_weights)
    masks = _masks(decisions, 7)
    h = rows.expand(xl)
    layers, pooled, win = [], None, None
    for i in range(7):
        W, b, gamma, beta = P[4 * i:4 * i + 4]
        if i == 5:
            if mode == "src":
                s = rows.expand_groups(seml).repeat_interleave(group_rows, dim=0)
            else:
                s = rows.expand(seml)
            h = torch.cat([h, s], dim=1)
        Y = h @ _w2(W).t() + b
        h, rec = _bn_layer(Y, ACT_ENC, gamma, beta, _running(running, i, Y.shape[1], dtype), training, eps, momentum,
                           masks[i], rows)
        layers.append(rec)
        if i == 5:
            pooled, win = _pool(h, rows, _winners(decisions))
    pp = h @ _w2(P[28]).t() + P[29]
    code = pooled @ P[30].t() + P[31]
    return Ref((rows.stored_groups(code), rows.stored(pp)), layers, win, {"x": xl, "sem": seml}, P)


def residual_ref(params, pp, code, code_first, grouping, *, training=True, eps=BN_EPS, momentum=BN_MOMENTUM,
                 running=None, decisions=None, row_weights=None, dtype=torch.float64):
    """ResidualNetFn: pp [M, Cp], code [G, Cc]; grouping: fixed rows per group (int) or gidx [M]
    (row -> group); ignored when Cc = 0. Output (out [M, 3 (any)],)."""
    assert len(params) == 14
    P = [_leaf(p, dtype) for p in params]
    ppl, codel = _leaf(pp, dtype), _leaf(code, dtype)
    M, Cc = ppl.shape[0], codel.shape[1]
    fixed = isinstance(grouping, int)
    assert row_weights is None or fixed
    rows = _Rows(M, grouping if fixed and row_weights is not None else 0, row_weights)
    masks = _masks(decisions, 3)
    h = rows.expand(ppl)
    if Cc > 0:
        if fixed:
            c = rows.expand_groups(codel).repeat_interleave(grouping, dim=0) if rows.weighted else \
                codel.repeat_interleave(grouping, dim=0)
        else:
            c = codel[grouping.detach().cpu().long()]
        h = torch.cat([c, h] if code_first else [h, c], dim=1)
    layers = []
    for i in range(3):
        W, b, gamma, beta = P[4 * i:4 * i + 4]
        Y = h @ _w2(W).t() + b
        h, rec = _bn_layer(Y, ACT_RES, gamma, beta, _running(running, i, Y.shape[1], dtype), training, eps, momentum,
                           masks[i], rows)
        layers.append(rec)
    out = h @ _w2(P[12]).t() + P[13]
    return Ref((rows.stored(out),), layers, None, {"pp": ppl, "code": codel}, P)


def chain_ref(params, x, acts, group_rows, pool=True, want_act=False, *, training=True, eps=BN_EPS,
              momentum=BN_MOMENTUM, running=None, decisions=None, row_weights=None, dtype=torch.float64):
    """PointChainFn: x [M, Cin], acts per layer (ACT_ENC, or ACT_BN for the last). Outputs
    (pooled [G, N_L] or None, act [M, N_L] or None)."""
    L = len(acts)
    assert len(params) == 4 * L and all(a == ACT_ENC for a in acts[:-1]) and acts[-1] in (ACT_ENC, ACT_BN)
    P = [_leaf(p, dtype) for p in params]
    xl = _leaf(x, dtype, grad=x.requires_grad)
    rows = _Rows(xl.shape[0], group_rows, row_weights)
    masks = _masks(decisions, L)
    h = rows.expand(xl)
    layers = []
    for i in range(L):
        W, b, gamma, beta = P[4 * i:4 * i + 4]
        Y = h @ _w2(W).t() + b
        h, rec = _bn_layer(Y, acts[i], gamma, beta, _running(running, i, Y.shape[1], dtype), training, eps, momentum,
                           masks[i], rows)
        layers.append(rec)
    pooled = win = None
    if pool:
        pooled, win = _pool(h, rows, _winners(decisions))
        pooled = rows.stored_groups(pooled)
    return Ref((pooled, rows.stored(h) if want_act else None), layers, win, {"x": xl}, P)


# ----------------------------------------------------------------------------------------------
# The chain cases of tests/test_chain_gpu.py, built on the CPU from a seed per case, so that
# tests/test_chain_ref.py can measure the restatement's own fp32 noise on exactly those inputs.
# Rows: G = 3 groups of 128 (pooling fused in the GEMM epilogue, group sums from per-block
# partials, row weights allowed) or G = 2 groups of 130 (groups straddle 128-row blocks, a ragged
# last block). Width sets are named by the GEMM kernel they force: "aligned" (multiples of 16, both
# <= 64 and > 64), "vec" (multiples of 4, not of 16; the tgt-mode semantic split at 72, off the
# 32 boundary), "scalar" (odd widths).
# ----------------------------------------------------------------------------------------------
ENC_WIDTHS = {          # (mlp1 + mlp2 widths after the 3 input channels), S, fuse_sem width, C
    "aligned": ((16, 16, 16, 32, 64), 16, 80, 16),
    "vec": ((8, 12, 8, 24, 72), 12, 72, 12),
    "scalar": ((5, 7, 10, 33, 45), 3, 45, 6),
}
RES_WIDTHS = {          # Cp, Cc, n1, n2, n3, out
    "real": (64, 64, 256, 256, 32, 3),
    "odd": (10, 7, 33, 20, 5, 3),
}
CHAIN_WIDTHS = {
    "aligned": (16, 32, 80),
    "vec": (8, 12, 72),
    "scalar": (5, 7, 33),
}
RAGGED_OFF = [0, 100, 101, 350, 350, 384]       # a one-row group and an empty group
ROW_W = (1, 3, 2)
MASK_CAP = 5e-4         # at most 0.05 % of a layer's ReLU decisions may differ between two precisions


def _case(fn, name, **kw):
    d = dict(fn=fn, name=f"{fn}-{name}", training=True, rw=False, use=None, seed=0)
    d.update(kw)
    return d


def _cases():
    c = []
    for mode in ("src", "tgt"):
        for gr in (128, 130):
            for ws in ("aligned", "vec", "scalar"):
                c.append(_case("enc", f"{mode}-{gr}-{ws}", mode=mode, gr=gr, widths=ws))
    c.append(_case("enc", "src-128-aligned-rw", mode="src", gr=128, widths="aligned", rw=True))
    c.append(_case("enc", "src-128-scalar-rw", mode="src", gr=128, widths="scalar", rw=True))
    c.append(_case("enc", "src-130-scalar-dcode-only", mode="src", gr=130, widths="scalar", use=(True, False)))
    c.append(_case("enc", "tgt-128-vec-dpp-only", mode="tgt", gr=128, widths="vec", use=(False, True)))
    c.append(_case("enc", "tgt-130-vec-eval", mode="tgt", gr=130, widths="vec", training=False))
    for ws in ("real", "odd"):
        for cf in (False, True):
            for grouping in (128, 130, "ragged"):
                c.append(_case("res", f"{ws}-{'codefirst' if cf else 'ppfirst'}-{grouping}", widths=ws, code_first=cf,
                               grouping=grouping))
        c.append(_case("res", f"{ws}-nocode", widths=ws, code_first=False, grouping="none"))
        c.append(_case("res", f"{ws}-128-rw", widths=ws, code_first=ws == "odd", grouping=128, rw=True))
    c.append(_case("res", "odd-codefirst-130-eval", widths="odd", code_first=True, grouping=130, training=False))
    E, B = ACT_ENC, ACT_BN
    for gr in (128, 130):
        for ws in ("aligned", "vec", "scalar"):
            c.append(_case("chain", f"{ws}-{gr}-pool", cin=3, widths=CHAIN_WIDTHS[ws], acts=(E, E, E), gr=gr, pool=True,
                           want_act=False))
    A = CHAIN_WIDTHS["aligned"]
    c.append(_case("chain", "bnlast-128-pool", cin=3, widths=A, acts=(E, E, B), gr=128, pool=True, want_act=False))
    c.append(_case("chain", "bnlast-130-both", cin=3, widths=CHAIN_WIDTHS["scalar"], acts=(E, E, B), gr=130, pool=True,
                   want_act=True))
    c.append(_case("chain", "act-only-130", cin=3, widths=CHAIN_WIDTHS["vec"], acts=(E, E, E), gr=130, pool=False,
                   want_act=True))
    c.append(_case("chain", "both-128", cin=3, widths=A, acts=(E, E, E), gr=128, pool=True, want_act=True))
    c.append(_case("chain", "both-128-dpooled-only", cin=3, widths=A, acts=(E, E, E), gr=128, pool=True, want_act=True,
                   use=(True, False)))
    c.append(_case("chain", "both-130-dact-only", cin=3, widths=A, acts=(E, E, E), gr=130, pool=True, want_act=True,
                   use=(False, True)))
    c.append(_case("chain", "cin64-128-pool", cin=64, widths=(32, 16, 80), acts=(E, E, E), gr=128, pool=True,
                   want_act=False))
    c.append(_case("chain", "cin64-130-both", cin=64, widths=(33, 20, 45), acts=(E, E, B), gr=130, pool=True,
                   want_act=True))
    c.append(_case("chain", "L1-128-both", cin=3, widths=(80,), acts=(E,), gr=128, pool=True, want_act=True))
    c.append(_case("chain", "L1-130-cin64-pool", cin=64, widths=(33,), acts=(E,), gr=130, pool=True, want_act=False))
    c.append(_case("chain", "xnograd-128-pool", cin=3, widths=A, acts=(E, E, E), gr=128, pool=True, want_act=False,
                   x_grad=False))
    for i, d in enumerate(c):
        d["seed"] = 1000 + i
    return c


CASES = _cases()
CASE_IDS = [c["name"] for c in CASES]


def _layer_params(g, n, k, conv=True, bn=True):
    bound = 1.0 / k ** 0.5
    W = (torch.rand(n, k, generator=g) * 2 - 1) * bound
    out = [W.unsqueeze(-1) if conv else W, (torch.rand(n, generator=g) * 2 - 1) * bound]
    if bn:
        out += [1.0 + 0.3 * (torch.rand(n, generator=g) * 2 - 1), 0.3 * (torch.rand(n, generator=g) * 2 - 1)]
    return out


def _run_stats(g, widths):
    """Non-trivial starting running statistics (and num_batches_tracked) of each BN layer."""
    return [(0.1 * torch.randn(n, generator=g), 0.5 + torch.rand(n, generator=g), 3 + i) for i, n in enumerate(widths)]


def make_case(case):
    """Inputs of one case as float32 CPU tensors: dict(params, inputs {name: tensor}, running
    [(rm, rv, nbt)], gout (output gradients, summed over copies for a unique-row case; None for
    an unused output), M, G, row_weights or None) plus the Function-specific fields."""
    g = torch.Generator().manual_seed(case["seed"])
    d = dict(row_weights=torch.tensor(ROW_W, dtype=torch.float32) if case["rw"] else None)
    fn = case["fn"]
    if fn == "enc":
        w5, S, Fw, C = ENC_WIDTHS[case["widths"]]
        gr = case["gr"]
        G = 3 if gr == 128 else 2
        M = G * gr
        dims = [(w5[0], 3), (w5[1], w5[0]), (w5[2], w5[1]), (w5[3], w5[2]), (w5[4], w5[3]), (Fw, w5[4] + S), (C, Fw)]
        params = []
        for n, k in dims:
            params += _layer_params(g, n, k)
        params += _layer_params(g, C, C, bn=False) + _layer_params(g, C, Fw, conv=False, bn=False)
        d.update(params=params, bn_widths=[n for n, _ in dims], M=M, G=G,
                 inputs=dict(x=torch.randn(M, 3, generator=g),
                             sem=torch.randn(G if case["mode"] == "src" else M, S, generator=g)),
                 gout=[torch.randn(G, C, generator=g), torch.randn(M, C, generator=g)])
    elif fn == "res":
        Cp, Cc, n1, n2, n3, no = RES_WIDTHS[case["widths"]]
        grouping = case["grouping"]
        if grouping == "none":
            Cp, Cc = Cp + Cc, 0
        if grouping == "ragged":
            off = torch.tensor(RAGGED_OFF)
            M, G = int(off[-1]), len(RAGGED_OFF) - 1
            d.update(off=off.int(), gidx=torch.repeat_interleave(torch.arange(G), off[1:] - off[:-1]).int())
        elif grouping == "none":
            M, G = 260, 1
        else:
            G = 3 if grouping == 128 else 2
            M = G * grouping
        dims = [(n1, Cp + Cc), (n2, n1), (n3, n2)]
        params = []
        for n, k in dims:
            params += _layer_params(g, n, k)
        params += _layer_params(g, no, n3, bn=False)
        d.update(params=params, bn_widths=[n for n, _ in dims], M=M, G=G,
                 inputs=dict(pp=torch.randn(M, Cp, generator=g), code=torch.randn(G, Cc, generator=g)),
                 gout=[torch.randn(M, no, generator=g)])
    else:
        gr, widths = case["gr"], case["widths"]
        G = 3 if gr == 128 else 2
        M = G * gr
        params, k = [], case["cin"]
        for n in widths:
            params += _layer_params(g, n, k)
            k = n
        x = torch.randn(M, case["cin"], generator=g)
        x.requires_grad_(case.get("x_grad", True))
        d.update(params=params, bn_widths=list(widths), M=M, G=G, inputs=dict(x=x),
                 gout=[torch.randn(G, widths[-1], generator=g) if case["pool"] else None,
                       torch.randn(M, widths[-1], generator=g) if case["want_act"] else None])
    if case["use"] is not None:
        d["gout"] = [t if u else None for t, u in zip(d["gout"], case["use"])]
    d["running"] = _run_stats(g, d["bn_widths"])
    return d


def run_case(case, data, dtype=torch.float64, decisions=None):
    """The reference on one case's inputs."""
    kw = dict(training=case["training"], running=data["running"], decisions=decisions, row_weights=data["row_weights"],
              dtype=dtype)
    I = data["inputs"]
    if case["fn"] == "enc":
        return encoder_ref(data["params"], I["x"], I["sem"], case["mode"], case["gr"], **kw)
    if case["fn"] == "res":
        gp = case["grouping"]
        grouping = data["gidx"].long() if gp == "ragged" else (data["M"] if gp == "none" else gp)
        return residual_ref(data["params"], I["pp"], I["code"], case["code_first"], grouping, **kw)
    return chain_ref(data["params"], I["x"], case["acts"], case["gr"], case["pool"], case["want_act"], **kw)


def pre_activation(layer):
    """The values a layer's ReLU decides on: z for Conv->BN->ReLU, the raw Y for Conv->ReLU->BN."""
    return layer["Y"] if layer["act"] == ACT_RES else layer["z"]
