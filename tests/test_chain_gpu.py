"""The three fused MLP chains (ured_hip/mlp.py: PointEncoderFn, ResidualNetFn, PointChainFn) called
directly and held, layer by layer, to the float64 restatement tests/chain_ref.py (pinned on the CPU
by tests/test_chain_ref.py), at the shapes where the chain glue takes each of its paths: 128-row
groups (pooling fused in the GEMM, group sums from block partials, three-way wgrad split, row
weights) and 130-row groups (pool_rows, direct group_colsum, a ragged last block); widths that
force the aligned gemm2_kernel, the vectorised gemm_kernel and the scalar gemm_kernel.

Per case:
  forward    every saved Y_i, every BN state (mean, invstd, scale, shift), the running statistics,
             num_batches_tracked and the outputs against the float64 run on its own decisions;
  decisions  the GPU's ReLU masks, recomputed from its saved Y_i and state, and its pool winners
             (saved argidx) may differ from float64's own only where the value decided on lies
             within that layer's forward tolerance of 0 (twice that, of the maximum, for a winner),
             and in at most MASK_CAP (0.05 %) of a layer's elements;
  backward   fixed random output gradients; float64 with the GPU's decisions forced; every input
             and parameter gradient as a whole tensor, elementwise;
  zero-gradient biases (a conv bias feeding a training-mode BN) bounded against the layer's
             weight gradient instead of being compared with noise;
  determinism  a second run is bitwise equal, outputs and gradients.

Every tolerance is  err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|  (the idiom of
tests/test_attn_gpu.py), ref32 the same restatement in float32 on the CPU (for the backward with
the same forced decisions), f = 1e-5 forward and 2e-5 for gradients as in tests/test_node_gpu.py;
zero-gradient biases: max|g_gpu| <= 3 * max|g_ref32| + 1e-5 * max|dW_ref64|. Nothing is derived
from the GPU's output. The ReLU mask of a Conv->BN->ReLU layer is recomputed as the sign of
Y * scale + shift evaluated in float64 from the GPU's fp32 Y, scale and shift: the product of two
fp32 numbers is exact there, so this is the sign of the kernels' own fmaf(Y, scale, shift).
"""
import pytest
import torch

import chain_ref as CR
from step_parity import report

pytestmark = pytest.mark.gpu

F_FWD, F_GRAD, FLOOR_MULT = 1e-5, 2e-5, 3.0
WORST = {}          # (chain, "forward" | "backward") -> (worst err / tolerance, what)


@pytest.fixture(scope="module")
def hip(dev):
    from ured_hip import kernels, mlp
    assert (kernels.ACT_ENC, kernels.ACT_RES, kernels.ACT_BN) == (CR.ACT_ENC, CR.ACT_RES, CR.ACT_BN)
    return mlp, kernels


def _d(t):
    return t.detach().double().cpu()


def _tol(r32, r64, f):
    r32, r64 = _d(r32), _d(r64)
    return FLOOR_MULT * (r32 - r64).abs().max().item() + f * r64.abs().max().item()


def check(case, phase, what, got, r32, r64, f):
    got, r64 = _d(got), _d(r64)
    assert got.shape == r64.shape, (case["name"], what, got.shape, r64.shape)
    if got.numel() == 0:
        return
    err, tol = (got - r64).abs().max().item(), _tol(r32, r64, f)
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    key = (case["fn"], phase)
    if ratio > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (ratio, f"{case['name']} {what}")
    print(f"{case['name']:34s} {phase:8s} {what:18s} err {err:.3e} tol {tol:.3e} ratio {ratio:.3f}")
    assert err <= tol, f"{case['name']} {what}: err {err:.3e} > 3 x fp32 floor + {f:.0e} x max = {tol:.3e}"


class Run:
    """One GPU run of a case: outputs, the autograd node's saved intermediates, the BN modules."""


def gpu_forward(case, data, dev, hip):
    mlp, K = hip
    r = Run()
    r.params = [p.to(dev).requires_grad_(True) for p in data["params"]]
    r.bns = []
    for n, (rm, rv, nbt) in zip(data["bn_widths"], data["running"]):
        bn = torch.nn.BatchNorm1d(n, eps=CR.BN_EPS, momentum=CR.BN_MOMENTUM).to(dev)
        with torch.no_grad():
            bn.running_mean.copy_(rm), bn.running_var.copy_(rv), bn.num_batches_tracked.fill_(nbt)
        r.bns.append(bn)
    fn, tr = case["fn"], case["training"]
    I = {k: v.detach().to(dev) for k, v in data["inputs"].items()}
    rw = K.RowWeights(data["row_weights"].to(dev), case["gr"] if fn != "res" else case["grouping"]) if case["rw"] else None
    r.leaves = {}
    with torch.enable_grad() if tr else torch.no_grad():
        if fn == "enc":
            spec = mlp.EncoderSpec(case["mode"], case["gr"], tr, r.bns, rw=rw)
            r.outs = mlp.PointEncoderFn.apply(spec, I["x"], I["sem"], *r.params)
        elif fn == "res":
            gp = case["grouping"]
            r.leaves = {"pp": I["pp"].requires_grad_(True)}
            if I["code"].numel():
                r.leaves["code"] = I["code"].requires_grad_(True)
            gidx = off = None
            group_rows = data["M"] if gp == "none" else gp
            if gp == "ragged":
                gidx, off, group_rows = data["gidx"].to(dev), data["off"].to(dev), 0
            spec = mlp.ResidualSpec(case["code_first"], gidx, off, group_rows, tr, r.bns, rw)
            r.outs = (mlp.ResidualNetFn.apply(spec, I["pp"], I["code"], *r.params),)
        else:
            if case.get("x_grad", True):
                r.leaves = {"x": I["x"].requires_grad_(True)}
            spec = mlp.ChainSpec(list(case["acts"]), case["gr"], tr, r.bns, pool=case["pool"], want_act=case["want_act"])
            p, a = mlp.PointChainFn.apply(spec, I["x"], *r.params)
            r.outs = (p if case["pool"] else None, a if case["want_act"] else None)
    if not tr:
        return r
    node = next(o for o in r.outs if o is not None and o.grad_fn is not None).grad_fn
    saved, nbn = node.saved_tensors, len(r.bns)
    first = {"enc": 4, "res": 2, "chain": 2}[fn]
    r.Ys = [saved[first + i] for i in range(nbn)]
    r.states = node.states
    r.argidx = saved[3] if fn == "enc" else (saved[1] if fn == "chain" else None)
    assert all(s is p for s, p in zip(saved[first + nbn:], r.params)) or \
        all(torch.equal(s, p) for s, p in zip(saved[first + nbn:], r.params))
    return r


def gpu_backward(case, data, dev, r):
    outs, gs = [], []
    for o, g in zip(r.outs, data["gout"]):
        if o is not None and g is not None:
            outs.append(o)
            gs.append(g.to(dev))
    names = list(r.leaves)
    got = torch.autograd.grad(outs, [r.leaves[k] for k in names] + r.params, gs, allow_unused=True)
    return dict(zip(names, got[:len(names)])), list(got[len(names):])


def gpu_decisions(case, data, r):
    """The GPU's ReLU masks (from its saved Y and BN state) and pool winners (point within group)."""
    masks = []
    for i, (Y, st) in enumerate(zip(r.Ys, r.states)):
        act = CR.ACT_RES if case["fn"] == "res" else (CR.ACT_ENC if case["fn"] == "enc" else case["acts"][i])
        if act == CR.ACT_RES:
            masks.append((Y > 0).cpu())
        elif act == CR.ACT_ENC:
            masks.append((Y.double() * st.scale.double() + st.shift.double() > 0).cpu())
        else:
            masks.append(None)
    win = None
    if r.argidx is not None:
        gr = case["gr"]
        win = r.argidx.long().cpu() - gr * torch.arange(r.argidx.shape[0]).unsqueeze(1)
        assert bool(((win >= 0) & (win < gr)).all()), f"{case['name']}: a pool winner outside its group"
    return {"masks": masks, "winners": win}


def check_forward(case, data, r, r32, r64):
    outs = [o for o in r.outs]
    for i, (o, a, b) in enumerate(zip(outs, r32.outputs, r64.outputs)):
        assert (o is None) == (b is None)
        if o is not None:
            check(case, "forward", f"output{i}", o, a, b, F_FWD)
    if not case["training"]:
        for bn, (rm, rv, nbt) in zip(r.bns, data["running"]):     # eval: the modules are left alone
            assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv)
            assert int(bn.num_batches_tracked) == nbt
        return
    for i, (Y, st, bn) in enumerate(zip(r.Ys, r.states, r.bns)):
        L32, L64 = r32.layers[i], r64.layers[i]
        check(case, "forward", f"Y{i}", Y, L32["Y"], L64["Y"], F_FWD)
        for k in ("mean", "invstd", "scale", "shift"):
            check(case, "forward", f"{k}{i}", getattr(st, k), L32[k], L64[k], F_FWD)
        check(case, "forward", f"running_mean{i}", bn.running_mean, L32["running_mean"], L64["running_mean"], F_FWD)
        check(case, "forward", f"running_var{i}", bn.running_var, L32["running_var"], L64["running_var"], F_FWD)
        assert int(bn.num_batches_tracked) == L64["num_batches_tracked"] == data["running"][i][2] + 1


def check_decisions(case, dec, r32, r64):
    """A GPU decision may differ from float64's own only on a value within the forward tolerance of
    the threshold, and only in MASK_CAP of a layer's elements."""
    pooled_layer = {"enc": 5, "res": None, "chain": len(r64.layers) - 1}[case["fn"]]
    for i, (m, L32, L64) in enumerate(zip(dec["masks"], r32.layers, r64.layers)):
        pre32, pre64 = CR.pre_activation(L32), CR.pre_activation(L64).detach()
        tol = _tol(pre32, pre64, F_FWD)
        if m is not None:
            diff = m != L64["mask"]
            n = int(diff.sum())
            print(f"{case['name']:34s} layer {i}: {n} of {m.numel()} masks differ from float64")
            assert n <= CR.MASK_CAP * m.numel(), f"{case['name']} layer {i}: {n} of {m.numel()} ReLU masks differ"
            if n:
                worst = pre64[diff].abs().max().item()
                assert worst <= tol, f"{case['name']} layer {i}: a mask differs where |z| = {worst:.3e} > {tol:.3e}"
        if i == pooled_layer and dec["winners"] is not None:
            L = L64
            h = (L["z"] * L["mask"].to(L["z"].dtype) if L["mask"] is not None else L["z"]).detach()
            hg = h.view(dec["winners"].shape[0], -1, h.shape[1])
            mx = hg.amax(dim=1)
            chosen = hg.gather(1, dec["winners"].unsqueeze(1)).squeeze(1)
            gap = (mx - chosen).max().item()
            print(f"{case['name']:34s} pool: {int((dec['winners'] != r64.winners).sum())} winners differ, "
                  f"largest gap {gap:.3e} (allowed {2 * tol:.3e})")
            assert gap <= 2 * tol, f"{case['name']}: a pool winner lies {gap:.3e} below the maximum (> {2 * tol:.3e})"


def zero_bias_indices(case):
    """Conv biases that feed a training-mode BN directly: exactly zero true gradient."""
    if case["fn"] == "res":
        return set()
    return {4 * i + 1 for i in range(7 if case["fn"] == "enc" else len(case["acts"]))}


def check_backward(case, gin, gpar, ref32, ref64):
    (i32, p32), (i64, p64) = ref32, ref64
    for k, g in gin.items():
        assert g is not None, f"{case['name']}: no gradient for {k}"
        check(case, "backward", f"d{k}", g, i32[k], i64[k], F_GRAD)
    zb = zero_bias_indices(case)
    for j, g in enumerate(gpar):
        assert g is not None, f"{case['name']}: no gradient for parameter {j}"
        a, b = p32[j], p64[j]
        a = torch.zeros_like(g, dtype=torch.float32, device="cpu") if a is None else a      # no path from the used output
        b = torch.zeros_like(g, dtype=torch.float64, device="cpu") if b is None else b
        if j in zb:
            dW = p64[j - 1]
            lim = FLOOR_MULT * a.abs().max().item() + 1e-5 * (0.0 if dW is None else dW.abs().max().item())
            got = g.abs().max().item()
            print(f"{case['name']:34s} backward zero-grad bias {j}: {got:.3e} (allowed {lim:.3e})")
            assert got <= lim, f"{case['name']} parameter {j} (zero true gradient): {got:.3e} > {lim:.3e}"
            continue
        check(case, "backward", f"param{j}", g, a.reshape(g.shape), b.reshape(g.shape), F_GRAD)


@pytest.mark.parametrize("name", CR.CASE_IDS)
def test_chain_case(dev, hip, name):
    case = CR.CASES[CR.CASE_IDS.index(name)]
    data = CR.make_case(case)
    r64, r32 = CR.run_case(case, data), CR.run_case(case, data, torch.float32)
    r = gpu_forward(case, data, dev, hip)
    check_forward(case, data, r, r32, r64)
    if not case["training"]:
        r2 = gpu_forward(case, data, dev, hip)
        assert all(torch.equal(a, b) for a, b in zip(r.outs, r2.outs) if a is not None)
        return
    dec = gpu_decisions(case, data, r)
    check_decisions(case, dec, r32, r64)
    gin, gpar = gpu_backward(case, data, dev, r)
    if case["fn"] == "chain" and not case.get("x_grad", True):
        assert gin == {}            # dx is None: x is no leaf of the run
    f64, f32 = CR.run_case(case, data, decisions=dec), CR.run_case(case, data, torch.float32, decisions=dec)
    check_backward(case, gin, gpar, f32.grads(*data["gout"]), f64.grads(*data["gout"]))
    # determinism: a second run from fresh modules is bitwise the first
    r2 = gpu_forward(case, data, dev, hip)
    gin2, gpar2 = gpu_backward(case, data, dev, r2)
    for a, b in zip(r.outs, r2.outs):
        assert (a is None and b is None) or torch.equal(a, b), f"{name}: outputs differ between two runs"
    for a, b in list(zip(gpar, gpar2)) + [(gin[k], gin2[k]) for k in gin]:
        assert torch.equal(a, b), f"{name}: gradients differ between two runs"
    for a, b in zip(r.bns, r2.bns):
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)


def test_chain_x_without_grad_gets_none(dev, hip):
    """PointChainFn returns dx = None for an x that does not require grad."""
    case = CR.CASES[CR.CASE_IDS.index("chain-xnograd-128-pool")]
    data = CR.make_case(case)
    r = gpu_forward(case, data, dev, hip)
    assert r.leaves == {} and r.outs[0].grad_fn.needs_input_grad[1] is False
    (r.outs[0] * data["gout"][0].to(dev)).sum().backward()
    assert all(p.grad is not None for p in r.params)


@pytest.mark.parametrize("name", ["enc-tgt-130-vec-eval", "res-odd-codefirst-130-eval", "chain-aligned-128-pool"])
def test_eval_mode_refuses_backward(dev, hip, name):
    """_layer_bwd is the batch-statistics BN backward; a chain that ran with training=False under
    autograd must not return that formula for the eval-BN gradient: its backward raises."""
    case = dict(CR.CASES[CR.CASE_IDS.index(name)], training=False)
    data = CR.make_case(case)
    mlp, K = hip
    params = [p.to(dev).requires_grad_(True) for p in data["params"]]
    bns = [torch.nn.BatchNorm1d(n).to(dev).eval() for n in data["bn_widths"]]
    I = {k: v.detach().to(dev) for k, v in data["inputs"].items()}
    if case["fn"] == "enc":
        out = mlp.PointEncoderFn.apply(mlp.EncoderSpec(case["mode"], case["gr"], False, bns), I["x"], I["sem"], *params)[1]
    elif case["fn"] == "res":
        spec = mlp.ResidualSpec(case["code_first"], None, None, case["grouping"], False, bns, None)
        out = mlp.ResidualNetFn.apply(spec, I["pp"].requires_grad_(True), I["code"], *params)
    else:
        spec = mlp.ChainSpec(list(case["acts"]), case["gr"], False, bns, pool=True, want_act=False)
        out = mlp.PointChainFn.apply(spec, I["x"], *params)[0]
    with pytest.raises(RuntimeError, match="training=False"):
        out.sum().backward()
    assert all(p.grad is None for p in params)


def test_report_worst_ratios():
    """Not a check: the worst err / tolerance the cases above measured, per chain (1.0 = at the
    tolerance), into the warnings summary."""
    names = {"enc": "PointEncoderFn", "res": "ResidualNetFn", "chain": "PointChainFn"}
    for (fn, phase), (ratio, what) in sorted(WORST.items()):
        report(f"chain parity {names[fn]} {phase}: worst err / tolerance {ratio:.3f} ({what})")
