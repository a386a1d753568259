"""Pins tests/chain_ref.py, the float64 restatement that tests/test_chain_gpu.py holds the fused
MLP chains to: against the oracle's target_encoder / residual_net (themselves pinned to the
reference by tests/test_oracle_golden.py), against torch.nn Conv1d / BatchNorm1d / max stacks, and
against itself (forced decisions, row weights, eval mode). The last test measures the
restatement's own fp32 noise on every GPU case, so that the seeds are fixed here, on the CPU."""
import pytest
import torch

import chain_ref as CR
from oracle import ured_ref

RTOL = 1e-12        # float64 rounding level, of each tensor's maximum

ENC_CONV = ("mlp1.0", "mlp1.3", "mlp2.0", "mlp2.3", "mlp2.6", "fuse_sem.0", "per_point_out.0")
ENC_BN = ("mlp1.1", "mlp1.4", "mlp2.1", "mlp2.4", "mlp2.7", "fuse_sem.1", "per_point_out.1")
RES_CONV, RES_BN = ("residual_net.0", "residual_net.3", "residual_net.6"), ("residual_net.2", "residual_net.5",
                                                                           "residual_net.8")


def by_name(name):
    return CR.CASES[CR.CASE_IDS.index(name)]


def close(a, b, what, scale=None):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel() == 0:
        return
    s = b.abs().max().item() if scale is None else scale
    err = (a - b).abs().max().item()
    assert err <= RTOL * s + 1e-300, f"{what}: {err:.3e} vs {RTOL:.0e} x {s:.3e}"


def oracle_dict(params, running, conv_names, bn_names, tail):
    """The Function's parameter list as the oracle's state_dict-keyed float64 dict (leaves)."""
    P, leaves = {}, []
    for i, (c, b) in enumerate(zip(conv_names, bn_names)):
        for key, t in zip((c + ".weight", c + ".bias", b + ".weight", b + ".bias"), params[4 * i:4 * i + 4]):
            P[key] = t.detach().double().clone().requires_grad_(True)
            leaves.append(P[key])
        rm, rv, nbt = running[i]
        P[b + ".running_mean"], P[b + ".running_var"] = rm.double().clone(), rv.double().clone()
    n = 4 * len(conv_names)
    for j, key in enumerate(tail):
        P[key] = params[n + j].detach().double().clone().requires_grad_(True)
        leaves.append(P[key])
    return P, leaves


def check_against(ref, gout, outs, gin, gpar, run_stats, zero_bias):
    """ref: a CR.Ref; the other implementation's outputs, input gradients {name: tensor},
    parameter gradients and running stats [(rm, rv)], from the same output gradients gout."""
    for i, (o, r) in enumerate(zip(outs, ref.outputs)):
        assert (o is None) == (r is None), i
        if o is not None:
            close(r, o, f"output {i}")
    rin, rpar = ref.grads(*gout)
    for k, v in gin.items():
        close(rin[k], v, f"d{k}")
    for j, (a, b) in enumerate(zip(rpar, gpar)):
        if b is None:       # unused output: no path to this parameter
            assert a is None or a.abs().max().item() == 0, j
            continue
        # an exactly-zero true gradient is rounding noise on both sides: of the weight gradient's size
        close(a, b, f"param grad {j}", scale=gpar[j - 1].abs().max().item() if j in zero_bias else None)
    for i, (rm, rv) in enumerate(run_stats):
        close(ref.layers[i]["running_mean"], rm, f"running_mean {i}")
        close(ref.layers[i]["running_var"], rv, f"running_var {i}")


def oracle_encoder(case, data):
    P, leaves = oracle_dict(data["params"], data["running"], ENC_CONV, ENC_BN,
                            ("per_point_out.3.weight", "per_point_out.3.bias", "fc.weight", "fc.bias"))
    G, gr = data["G"], case["gr"]
    x = data["inputs"]["x"].double().requires_grad_(True)
    sem = data["inputs"]["sem"].double().requires_grad_(True)
    src = case["mode"] == "src"
    xo = x.view(1, G, gr, 3) if src else x.view(G, gr, 3)
    so = sem.view(1, G, -1) if src else sem.view(G, gr, -1)
    code, pp = ured_ref.target_encoder(P, xo, so, src, training=case["training"])
    pp = pp.transpose(1, 2).reshape(G * gr, -1)
    gs = [(o, g.double()) for o, g in zip((code, pp), data["gout"]) if g is not None]
    got = torch.autograd.grad([o for o, _ in gs], [x, sem] + leaves, [g for _, g in gs], allow_unused=True)
    return (code, pp), {"x": got[0], "sem": got[1]}, list(got[2:]), [(P[b + ".running_mean"], P[b + ".running_var"])
                                                                   for b in ENC_BN]


def oracle_residual(case, data):
    P, leaves = oracle_dict(data["params"], data["running"], RES_CONV, RES_BN,
                            ("residual_net.9.weight", "residual_net.9.bias"))
    pp = data["inputs"]["pp"].double().requires_grad_(True)
    code = data["inputs"]["code"].double().requires_grad_(True)
    M, gp = data["M"], case["grouping"]
    if gp == "none":
        feat = pp
    else:
        gid = data["gidx"].long() if gp == "ragged" else torch.arange(M) // gp
        feat = torch.cat([code[gid], pp], 1) if case["code_first"] else torch.cat([pp, code[gid]], 1)
    out = ured_ref.residual_net(P, feat.unsqueeze(0), training=case["training"]).squeeze(0)
    got = torch.autograd.grad([out], [pp, code] + leaves, [data["gout"][0].double()], allow_unused=True)
    gin = {"pp": got[0]}
    if code.numel():
        gin["code"] = got[1]
    return (out,), gin, list(got[2:]), [(P[b + ".running_mean"], P[b + ".running_var"]) for b in RES_BN]


def nn_chain(case, data):
    """torch.nn Conv1d / BatchNorm1d / max stack of a PointChainFn case, in float64."""
    G, gr, L = data["G"], case["gr"], len(case["acts"])
    x = data["inputs"]["x"].detach().double().requires_grad_(data["inputs"]["x"].requires_grad)
    h = x.view(G, gr, -1).transpose(1, 2)
    leaves, bns = [], []
    k = case["cin"]
    for i, n in enumerate(case["widths"]):
        conv, bn = torch.nn.Conv1d(k, n, 1).double(), torch.nn.BatchNorm1d(n, eps=CR.BN_EPS, momentum=CR.BN_MOMENTUM).double()
        W, b, gamma, beta = data["params"][4 * i:4 * i + 4]
        rm, rv, nbt = data["running"][i]
        with torch.no_grad():
            conv.weight.copy_(W.reshape(n, k, 1)), conv.bias.copy_(b), bn.weight.copy_(gamma), bn.bias.copy_(beta)
            bn.running_mean.copy_(rm), bn.running_var.copy_(rv), bn.num_batches_tracked.fill_(nbt)
        bn.train(case["training"])
        h = bn(conv(h))
        if case["acts"][i] == CR.ACT_ENC:
            h = torch.relu(h)
        leaves += [conv.weight, conv.bias, bn.weight, bn.bias]
        bns.append(bn)
        k = n
    pooled = h.max(dim=2)[0] if case["pool"] else None
    act = h.transpose(1, 2).reshape(G * gr, -1) if case["want_act"] else None
    gs = [(o, g.double()) for o, g in zip((pooled, act), data["gout"]) if o is not None and g is not None]
    inp = [x] if x.requires_grad else []
    got = torch.autograd.grad([o for o, _ in gs], inp + leaves, [g for _, g in gs], allow_unused=True)
    gin = {"x": got[0]} if inp else {}
    gpar = [g.reshape(p.shape) if g is not None else None for g, p in zip(got[len(inp):], data["params"])]
    for i, bn in enumerate(bns):
        assert int(bn.num_batches_tracked) == data["running"][i][2] + int(case["training"])
    return (pooled, act), gin, gpar, [(bn.running_mean, bn.running_var) for bn in bns]


ORACLES = {"enc": oracle_encoder, "res": oracle_residual, "chain": nn_chain}
PLAIN = [c["name"] for c in CR.CASES if not c["rw"]]


def zero_bias_indices(case):
    """Parameter indices of the conv biases with an exactly zero true gradient (a bias feeding a
    training-mode BN directly): every BN layer of the encoder and of the point chain; none in
    the Conv->ReLU->BN residual net."""
    if case["fn"] == "res" or not case["training"]:
        return set()
    nbn = 7 if case["fn"] == "enc" else len(case["acts"])
    return {4 * i + 1 for i in range(nbn)}


@pytest.mark.parametrize("name", PLAIN)
def test_against_oracle(name):
    """Outputs, input gradients, parameter gradients, running statistics of every case without row
    weights (training and eval; both encoder modes; both concatenation orders, fixed / ragged
    groups with an empty one, Cc = 0; ACT_ENC / ACT_BN last layers, pool / act / both) against
    oracle.ured_ref (encoder, residual net) or a torch.nn stack (point chain), in float64."""
    case = by_name(name)
    data = CR.make_case(case)
    ref = CR.run_case(case, data)
    outs, gin, gpar, stats = ORACLES[case["fn"]](case, data)
    check_against(ref, data["gout"], outs, gin, gpar, stats, zero_bias_indices(case))
    for i, L in enumerate(ref.layers):
        assert L["num_batches_tracked"] == data["running"][i][2] + int(case["training"])


@pytest.mark.parametrize("name", ["enc-src-130-vec", "enc-tgt-128-scalar", "res-odd-codefirst-ragged",
                                  "chain-bnlast-130-both", "chain-both-128"])
def test_own_decisions_change_nothing(name):
    case = by_name(name)
    data = CR.make_case(case)
    for dtype in (torch.float64, torch.float32):
        a = CR.run_case(case, data, dtype)
        b = CR.run_case(case, data, dtype, decisions=a.decisions())
        for x, y in zip(a.outputs, b.outputs):
            assert (x is None and y is None) or torch.equal(x, y)
        for La, Lb in zip(a.layers, b.layers):
            for k in ("Y", "z", "mean", "invstd", "scale", "shift", "running_mean", "running_var"):
                assert torch.equal(La[k], Lb[k]), k
        (ia, pa), (ib, pb) = a.grads(*data["gout"]), b.grads(*data["gout"])
        for x, y in list(zip(pa, pb)) + [(ia[k], ib[k]) for k in ia]:
            assert (x is None and y is None) or torch.equal(x, y)


def test_forced_decisions_are_used():
    """A flipped mask element and a moved winner change the result (the override is not ignored),
    and the gradient is routed by the forced mask."""
    case = by_name("chain-both-128")
    data = CR.make_case(case)
    a = CR.run_case(case, data)
    dec = a.decisions()
    dec["masks"] = [m.clone() for m in dec["masks"]]
    dec["masks"][-1][5, 7] = ~dec["masks"][-1][5, 7]
    dec["winners"] = dec["winners"].clone()
    dec["winners"][1, 3] = (dec["winners"][1, 3] + 1) % case["gr"]
    b = CR.run_case(case, data, decisions=dec)
    assert torch.equal(b.decisions()["masks"][-1], dec["masks"][-1]) and torch.equal(b.winners, dec["winners"])
    assert b.outputs[1][5, 7].item() == (a.layers[-1]["z"][5, 7].item() if dec["masks"][-1][5, 7] else 0.0)
    assert b.outputs[0][1, 3].item() == b.outputs[1][128 + int(dec["winners"][1, 3]), 3].item()
    assert not torch.equal(a.grads(*data["gout"])[1][0], b.grads(*data["gout"])[1][0])


def _expanded(case, data):
    """The physically expanded batch of a unique-row case, with a random gradient per copy; the
    case's own gout becomes the sum over the copies."""
    w = [int(v) for v in data["row_weights"]]
    gr = case["gr"] if case["fn"] != "res" else case["grouping"]
    groups = torch.repeat_interleave(torch.arange(len(w)), torch.tensor(w))
    rows = (groups.unsqueeze(1) * gr + torch.arange(gr)).reshape(-1)
    g = torch.Generator().manual_seed(case["seed"] + 7)
    big = dict(data, row_weights=None, G=len(groups), M=len(rows))
    per_group = {"sem"} if case.get("mode") == "src" else {"code"}
    big["inputs"] = {k: (v[groups] if k in per_group else v[rows]) for k, v in data["inputs"].items()}
    big["gout"], summed = [], []
    for t in data["gout"]:
        if t is None:
            big["gout"].append(None), summed.append(None)
            continue
        idx = groups if t.shape[0] == len(w) else rows
        ge = torch.randn(len(idx), t.shape[1], generator=g, dtype=torch.float64)
        big["gout"].append(ge)
        summed.append(torch.zeros_like(t, dtype=torch.float64).index_add_(0, idx, ge))
    return big, summed, groups, rows, per_group


@pytest.mark.parametrize("name", ["enc-src-128-aligned-rw", "enc-src-128-scalar-rw", "res-real-128-rw",
                                  "res-odd-128-rw", "chain-both-128"])
def test_row_weights_equal_expanded_batch(name):
    case = by_name(name)
    data = CR.make_case(case)
    if data["row_weights"] is None:
        data["row_weights"] = torch.tensor(CR.ROW_W, dtype=torch.float32)
    big, summed, groups, rows, per_group = _expanded(case, data)
    a = CR.run_case(case, data)
    b = CR.run_case(case, big)
    first_g = torch.tensor([int((groups == i).nonzero()[0]) for i in range(data["G"])])
    gr = len(rows) // len(groups)
    first = (first_g.unsqueeze(1) * gr + torch.arange(gr)).reshape(-1)
    for x, y in zip(a.outputs, b.outputs):
        if x is not None:
            close(x, y[first_g] if x.shape[0] == data["G"] else y[first], "output")
    for La, Lb in zip(a.layers, b.layers):
        for k in ("mean", "invstd", "scale", "shift", "running_mean", "running_var"):
            close(La[k], Lb[k], k)
        close(La["Y"], Lb["Y"][first], "Y")
        assert La["num_batches_tracked"] == Lb["num_batches_tracked"]
    (ia, pa), (ib, pb) = a.grads(*summed), b.grads(*big["gout"])
    for j, (x, y) in enumerate(zip(pa, pb)):
        close(x, y, f"param grad {j}", scale=max(y.abs().max().item(), pb[j - 1].abs().max().item() if j % 4 == 1 else 0))
    for k in ia:
        if ia[k] is None:
            assert ib[k] is None
            continue
        idx = groups if k in per_group else rows
        close(ia[k], torch.zeros_like(ia[k]).index_add_(0, idx, ib[k]), f"d{k}")


def test_eval_mode_is_batch_norm_eval():
    """One layer of each kind against F.batch_norm(training=False), forward and backward."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    M, K, N = 50, 6, 9
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    W, b = torch.randn(N, K, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(N, generator=g, dtype=torch.float64) + 0.5, torch.randn(N, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(N, generator=g, dtype=torch.float64), torch.rand(N, generator=g, dtype=torch.float64) + 0.5
    go = torch.randn(M, N, generator=g, dtype=torch.float64)
    for act in (CR.ACT_ENC, CR.ACT_BN):
        ref = CR.chain_ref([W, b, gamma, beta], x.clone().requires_grad_(True), [act], M, pool=False, want_act=True,
                           training=False, running=[(rm, rv, 4)])
        leaves = [t.clone().requires_grad_(True) for t in (x, W, b, gamma, beta)]
        y = F.batch_norm(leaves[0] @ leaves[1].t() + leaves[2], rm.clone(), rv.clone(), leaves[3], leaves[4], False, 0.1,
                         CR.BN_EPS)
        y = torch.relu(y) if act == CR.ACT_ENC else y
        want = torch.autograd.grad(y, leaves, go)
        close(ref.outputs[1], y, "eval output")
        gin, gpar = ref.grads(None, go)
        for a, w_ in zip([gin["x"]] + gpar, want):
            close(a, w_, "eval grad")
        L = ref.layers[0]
        assert torch.equal(L["running_mean"], rm) and torch.equal(L["running_var"], rv) and L["num_batches_tracked"] == 4


def mask_disagreement(ref_a, ref_b):
    """Per BN layer with a ReLU: (elements whose mask differs, elements)."""
    out = []
    for La, Lb in zip(ref_a.layers, ref_b.layers):
        if La["mask"] is None:
            out.append((0, 1))
        else:
            out.append((int((La["mask"] != Lb["mask"]).sum()), La["mask"].numel()))
    return out


@pytest.mark.parametrize("name", CR.CASE_IDS)
def test_fp32_noise_floor_of_every_gpu_case(name):
    """The restatement alone, float32 against float64, on every case of tests/test_chain_gpu.py:
    plain fp32 rounding flips no more ReLU decisions than the cap that test puts on the GPU
    (MASK_CAP of a layer's elements), in any BN layer. A seed that violates this is replaced
    here, never after looking at a GPU result."""
    case = by_name(name)
    data = CR.make_case(case)
    r64, r32 = CR.run_case(case, data), CR.run_case(case, data, torch.float32)
    worst = 0.0
    for i, (n, tot) in enumerate(mask_disagreement(r64, r32)):
        assert n <= CR.MASK_CAP * tot, f"{name} layer {i}: {n} of {tot} fp32 masks differ from float64"
        z64, z32 = CR.pre_activation(r64.layers[i]), CR.pre_activation(r32.layers[i])
        worst = max(worst, (z32.double() - z64).abs().max().item() / z64.abs().max().item())
    assert worst <= 1e-4, f"{name}: fp32 pre-activations deviate {worst:.2e} of the layer maximum"
