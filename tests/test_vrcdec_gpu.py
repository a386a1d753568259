"""VRCNet's decoder on the GPU (the EF / fold kernels of csrc/vrc.hip, ured_hip/vrc.py, EF_expansion in
chamfer3D/model_utils.py, Folding and MSAP_SKN_decoder in models/vrcnet.py) against tests/vrcdec_ref.py in
float64, which tests/test_vrcdec_ref.py pins to the reference's own modules.

Tolerance and decisions exactly as in tests/test_vrc_gpu.py: err(gpu, ref64) <= 3 * err(ref32, ref64) +
f * max|ref64| (tests/tol_check.py; F_FWD forward, F_GRAD gradients); kNN / FPS / ranking indices are compared
exactly (the fixtures keep them away from a flip, tests/vrcdec_ref.py); a ReLU mask may differ from float64's
only within the layer's forward tolerance of zero and in at most MASK_CAP of the layer, a max slot within
twice the tolerance; the float64 backward runs with the GPU's decisions forced under fixed cotangents, whole
gradient tensors are compared, and a second run must give bitwise-equal gradients.
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import vrc_ref as R
import vrcdec_ref as D
from chain_ref import MASK_CAP
from tol_check import F_FWD, F_GRAD, FLOOR_MULT, check

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def V(dev):
    from ured_hip import vrc
    yield vrc
    for fam, (ratio, what) in sorted(WORST.items()):
        print(f"worst ratio {fam:14s} {ratio:.3f}  ({what})")


@pytest.fixture(autouse=True)
def _vrc_debug_word():
    """The debug build's bounds word of vrc.hip (file id 18), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_vrc"):
        return
    fn = mod._lib.ured_dbg_vrc
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): vrc.hip:{v & 0xFFFFFFFF}"


@pytest.fixture(scope="module")
def refs():
    """Computed once, shared, never modified."""
    return {(n, d): D.run_fixture(n, d) for n in ("ef", "fold", "dec_fold", "dec_ef") for d in (torch.float64, torch.float32)}


def _eighths(rng, shape, lo=-16, hi=17):
    return torch.from_numpy(rng.integers(lo, hi, size=shape).astype(np.float64) / 8)


def _normal(rng, shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) * scale


def _tol(a32, a64, f=F_FWD):
    return FLOOR_MULT * (a32.double() - a64).abs().max().item() + f * a64.abs().max().item()


def _mask_check(what, got, d32, d64, name, mult=1.0):
    pre64 = d64.pre[name]
    got = got.cpu().reshape(pre64.shape)
    tol = mult * _tol(d32.pre[name], pre64)
    diff = got != d64.mask[name]
    far = diff & (pre64.abs() >= tol)
    assert not bool(far.any()), f"{what} {name}: {int(far.sum())} masks differ beyond the forward tolerance {tol:.3e}"
    assert int(diff.sum()) <= MASK_CAP * diff.numel(), f"{what} {name}: {int(diff.sum())} of {diff.numel()} masks differ"
    return got


def _slot_check(what, got, d32, d64, name, pre):
    """A max slot may differ from float64's only where the winner's lead is within twice the forward tolerance."""
    want = d64.idx[name]
    got = got.cpu().long().reshape(want.shape)
    diff = got != want
    tol = 2 * _tol(d32.pre[pre], d64.pre[pre])
    assert not bool((diff & (d64.margin[name] >= tol)).any()), f"{what} {name}: a slot differs beyond twice the tolerance"
    assert int(diff.sum()) <= MASK_CAP * diff.numel(), f"{what} {name}: {int(diff.sum())} of {diff.numel()} slots differ"
    return got


def _masks(what, pre_gpu, d32, d64):
    return {name: _mask_check(what, pre_gpu[name].detach() > 0, d32, d64, name) for name in d64.mask}


def _ef_idx(rng, B, N, k):
    """As _sa_idx of tests/test_vrc_gpu.py: a duplicate in every row, a hub every row names, a point no row
    names, one index out of range."""
    idx = torch.from_numpy(rng.integers(0, N, size=(B, N, k))).int()
    idx[:, :, 0] = 0
    if k >= 3:
        idx[:, :, 2] = idx[:, :, 1]
    if N > 1:
        idx[idx == N - 1] = 0
    if k >= 2:
        idx[0, 0, k - 1] = N
    return idx


def _lone(idx, N):
    B = idx.shape[0]
    named = torch.zeros(B, N, dtype=torch.bool)
    ok = (idx >= 0) & (idx < N)
    for b in range(B):
        named[b, idx[b][ok[b]].long()] = True
    return ~named.view(-1)


# ---------------- the EF core with given idx ----------------

EF_CASES = [(1, 1, 1, 1, 1, 1), (1, 5, 4, 3, 8, 1), (2, 65, 4, 16, 8, 3), (1, 33, 4, 256, 64, 2), (2, 17, 4, 64, 256, 4),
            (1, 9, 8, 5, 64, 2), (2, 4, 4, 3, 8, 2)]       # the last: k = N, permutations


@pytest.mark.parametrize("B,N,k,C,O,r", EF_CASES)
def test_ef_core(V, dev, B, N, k, C, O, r):
    from chamfer3D.model_utils import EF_expansion
    rng = np.random.default_rng(B * 1000 + N * 10 + r)
    torch.manual_seed(N)
    mod = EF_expansion(C, O, r, k)
    Pr = {n: p.detach().clone() for n, p in mod.named_parameters()}
    mod = mod.to(dev)
    x = _normal(rng, (B * N, C))
    cot = torch.from_numpy(rng.standard_normal((B * N * r, O)))
    idxs = [_ef_idx(rng, B, N, k)]
    if k == N and N > 1:
        idxs.append(torch.stack([torch.stack([torch.from_numpy(rng.permutation(N)) for _ in range(N)]) for _ in range(B)]).int())
    for idx in idxs:
        def fn(P, xin, dec):
            return (D.ef_core(P, "", xin, idx, r, dec, "ef"),)
        r64, r32 = D.run(fn, Pr, [x]), D.run(fn, Pr, [x], dtype=torch.float32)
        xg = x.to(dev).requires_grad_(True)
        rec = {}
        out = mod.core_rows(xg, idx.to(dev), rec, "ef")
        what = f"ef {B}x{N} k{k} C{C} O{O} r{r}"
        assert tuple(out.shape) == (B * N * r, O)
        check(WORST, "ef_fwd", what, out, r32["outs"][0], r64["outs"][0], F_FWD)
        d32, d64 = r32["dec"], r64["dec"]
        force = _masks(what, rec["pre"], d32, d64)
        force["ef.slot"] = _slot_check(what, rec["slot"]["ef"], d32, d64, "ef.slot", "ef.H")
        f64, f32 = D.run(fn, Pr, [x], [cot], force=force), D.run(fn, Pr, [x], [cot], torch.float32, force)
        params = dict(mod.named_parameters())
        leaves = [xg] + list(params.values())
        grads = torch.autograd.grad((out * cot.float().to(dev)).sum(), leaves)
        for name, got in zip(["in0"] + list(params), grads):
            check(WORST, "ef_bwd", f"{what} d{name}", got, f32["grads"][name], f64["grads"][name], F_GRAD)
        again = torch.autograd.grad((mod.core_rows(xg, idx.to(dev)) * cot.float().to(dev)).sum(), leaves)
        assert all(torch.equal(a, b) for a, b in zip(grads, again))
        # the edge kernel alone: a point no row names gets exact zeros in the neighbour half
        W = O * r
        P = _normal(rng, (B * N, 2 * W)).to(dev).requires_grad_(True)
        G = _normal(rng, (B * N * k, W)).to(dev).requires_grad_(True)
        ce = _normal(rng, (B * N * k, W)).to(dev)
        dP, dG = torch.autograd.grad((V.EfEdgeFn.apply(P, idx.to(dev), G) * ce).sum(), [P, G])
        lone = _lone(idx, N)
        if bool(lone.any()):
            assert bool((dP[lone.to(dev), W:] == 0).all())
        dP2, = torch.autograd.grad((V.EfEdgeFn.apply(P, idx.to(dev)) * ce).sum(), [P])
        assert bool(torch.isfinite(dP2).all()) and bool(torch.isfinite(dG).all())


def test_ef_kernels_in_eighths_are_exact_and_the_lowest_slot_wins(V, dev):
    """Features in eighths: every sum is exact in both precisions, and a tie goes to the lowest j."""
    rng = np.random.default_rng(3)
    B, N, k, r, O = 2, 19, 4, 3, 10
    W = O * r
    idx = _ef_idx(rng, B, N, k)
    P, G = _eighths(rng, (B * N, 2 * W), -4, 5), _eighths(rng, (B * N * k, W), -4, 5)
    cot = _eighths(rng, (B * N * k, W), -4, 5)

    def edge(Pd, Gd):
        Pv = Pd.view(B, N, 2 * W)
        nb = R.gather_rows(Pv[:, :, W:], idx)                                # [B, N, k, W]
        return torch.relu(Gd.view(B, N, k, W) + Pv[:, :, None, :W] + nb).reshape(B * N * k, W)
    P64, G64 = P.clone().requires_grad_(True), G.clone().requires_grad_(True)
    want = edge(P64, G64)
    wP, wG = torch.autograd.grad((want * cot).sum(), [P64, G64])
    Pg, Gg = P.float().to(dev).requires_grad_(True), G.float().to(dev).requires_grad_(True)
    got = V.EfEdgeFn.apply(Pg, idx.to(dev), Gg)
    assert torch.equal(got.detach().cpu().double(), want.detach())
    gP, gG = torch.autograd.grad((got * cot.float().to(dev)).sum(), [Pg, Gg])
    assert torch.equal(gP.cpu().double(), wP) and torch.equal(gG.cpu().double(), wG)
    # the max over the slots: few values, so ties in most columns; slot k - 1 repeats slot 0
    H = _eighths(rng, (B, N, k, r, O), -1, 2)
    H[:, :, k - 1] = H[:, :, 0]
    ch = _eighths(rng, (B * N * r, O))
    sl = R._first_max(H, 2)
    H64 = H.clone().requires_grad_(True)
    wmax = H64.gather(2, sl.unsqueeze(2)).squeeze(2).reshape(B * N * r, O)
    wH, = torch.autograd.grad((wmax * ch).sum(), [H64])
    Hg = H.float().reshape(B * N * k * r, O).to(dev).requires_grad_(True)
    out, slot = V.EfMaxFn.apply(Hg, B, N, k, r)
    assert slot.dtype == torch.uint8 and tuple(slot.shape) == (B * N * r, O)
    assert torch.equal(out.detach().cpu().double(), wmax.detach())
    assert torch.equal(slot.cpu().long().view(B, N, r, O), sl), "the lowest j must win a tie"
    gH, = torch.autograd.grad((out * ch.float().to(dev)).sum(), [Hg])
    assert torch.equal(gH.cpu().double().view(B, N, k, r, O), wH)


# ---------------- the fold kernel ----------------

@pytest.mark.parametrize("B,N,r,Co", [(1, 1, 1, 1), (2, 17, 3, 130), (1, 64, 4, 256)])
def test_fold_kernel(V, dev, B, N, r, Co):
    rng = np.random.default_rng(N * 10 + r)
    for exact in (False, True):
        U = _eighths(rng, (B * N, Co), -8, 9) if exact else _normal(rng, (B * N, Co)).double()
        T = _eighths(rng, (r, Co), -8, 9) if exact else _normal(rng, (r, Co)).double()
        cot = _eighths(rng, (B * N * r, Co), -8, 9) if exact else torch.from_numpy(rng.standard_normal((B * N * r, Co)))

        def fn(Pr, u, t, dec):
            return (torch.relu(u.unsqueeze(1) + t.unsqueeze(0)).reshape(B * N * r, Co),)
        r64, r32 = D.run(fn, {}, [U, T], [cot]), D.run(fn, {}, [U, T], [cot], torch.float32)
        g = [t.float().to(dev).requires_grad_(True) for t in (U, T)]
        out = V.FoldFn.apply(*g)
        grads = torch.autograd.grad((out * cot.float().to(dev)).sum(), g)
        what = f"fold {B}x{N} r{r} Co{Co}"
        if exact:
            assert torch.equal(out.detach().cpu().double(), r64["outs"][0])
            assert torch.equal(grads[0].cpu().double(), r64["grads"]["in0"])
            assert torch.equal(grads[1].cpu().double(), r64["grads"]["in1"])
        else:
            check(WORST, "fold", what, out, r32["outs"][0], r64["outs"][0], F_FWD)
            gm = out.detach().cpu() > 0                                      # the float64 backward under the GPU's mask
            pre64 = (U.unsqueeze(1) + T.unsqueeze(0)).reshape(B * N * r, Co)
            pre32 = (U.float().unsqueeze(1) + T.float().unsqueeze(0)).reshape(B * N * r, Co)
            diff = gm != (pre64 > 0)
            assert not bool((diff & (pre64.abs() >= _tol(pre32, pre64))).any())
            assert int(diff.sum()) <= MASK_CAP * diff.numel()

            def forced(Pr, u, t, dec):
                return ((u.unsqueeze(1) + t.unsqueeze(0)).reshape(B * N * r, Co) * gm.to(u.dtype),)
            f64, f32 = D.run(forced, {}, [U, T], [cot]), D.run(forced, {}, [U, T], [cot], torch.float32)
            check(WORST, "fold", f"{what} dU", grads[0], f32["grads"]["in0"], f64["grads"]["in0"], F_GRAD)
            check(WORST, "fold", f"{what} dT", grads[1], f32["grads"]["in1"], f64["grads"]["in1"], F_GRAD)
        again = torch.autograd.grad((V.FoldFn.apply(*g) * cot.float().to(dev)).sum(), g)
        assert all(torch.equal(a, b) for a, b in zip(grads, again))


# ---------------- modules ----------------

def _build(name, dev):
    from chamfer3D.model_utils import EF_expansion
    from models import vrcnet as M
    if name == "ef":
        E = D.EF
        mod = EF_expansion(E["C"], E["O"], E["r"], E["k"])
    elif name == "fold":
        Fo = D.FOLD
        mod = M.Folding(Fo["C"], Fo["output_size"], Fo["step_ratio"], Fo["G"])
    else:
        c = D.DECS[name]
        mod = M.MSAP_SKN_decoder(c["num_coarse_raw"], c["num_fps"], c["num_coarse"], c["num_fine"], c["layers"], c["knn_list"],
                                 c["pk"], c["points_label"], c["local_folding"], c["over_scale"], pts_num=c["pts_num"])
    mod.load_state_dict(D.fixture(name)[0], strict=True)                 # reference keys, strict
    return mod.to(dev).eval()


def _grads_check(what, name, mod, leaves_in, outs, force, fam, none=()):
    _, _, cots = D.fixture(name)
    f64, f32 = D.run_fixture(name, force=force), D.run_fixture(name, torch.float32, force)
    params = dict(mod.named_parameters())
    leaves = list(leaves_in) + list(params.values())
    loss = sum((o * c.float().to(o.device)).sum() for o, c in zip(outs, cots))
    got = torch.autograd.grad(loss, leaves, allow_unused=True)
    names = [f"in{i}" for i in range(len(leaves_in))] + list(params)
    for k, g in zip(names, got):
        if k.startswith(tuple(none)):
            assert g is None, f"{what}: {k} must take no gradient"
            assert k in f64["none"]
            continue
        assert g is not None, k
        check(WORST, fam, f"{what} d{k}", g, f32["grads"][k], f64["grads"][k], F_GRAD)
    return [g for g in got if g is not None]


def test_ef_expansion_module(V, dev, refs):
    r64, r32 = refs["ef", torch.float64], refs["ef", torch.float32]
    E = D.EF
    B, N = E["B"], E["N"]
    x = D.fixture("ef")[1][0]
    mod = _build("ef", dev)
    mod.decisions = {}
    xg = x.to(dev).requires_grad_(True)
    out = mod(xg)
    rec = mod.decisions
    assert tuple(out.shape) == (B, E["O"], N * E["r"])
    assert torch.equal(rec["knn"]["ef"].cpu().long(), r64["dec"].idx["ef.knn"]), "the feature-space kNN must match exactly"
    check(WORST, "ef_mod", "EF_expansion forward", out, r32["outs"][0], r64["outs"][0], F_FWD)
    del mod.decisions
    rows = mod.forward_rows(xg.transpose(1, 2).reshape(B * N, -1), B)
    assert torch.equal(rows.view(B, N * E["r"], E["O"]).transpose(1, 2).detach(), out.detach()), "forward and forward_rows must agree"
    force = _masks("ef", rec["pre"], r32["dec"], r64["dec"])
    force["ef.slot"] = _slot_check("ef", rec["slot"]["ef"], r32["dec"], r64["dec"], "ef.slot", "ef.H")
    force["ef.knn"] = rec["knn"]["ef"].cpu().long()
    _grads_check("ef", "ef", mod, [xg], [out], force, "ef_mod")


def test_folding_module(V, dev, refs):
    r64, r32 = refs["fold", torch.float64], refs["fold", torch.float32]
    Fo = D.FOLD
    x, g = D.fixture("fold")[1]
    mod = _build("fold", dev)
    assert "grid" not in mod.state_dict() and mod.grid.device.type == "cuda"
    mod.decisions = {}
    xg, gg = x.to(dev).requires_grad_(True), g.to(dev).requires_grad_(True)
    out = mod(xg, gg)
    assert tuple(out.shape) == (Fo["B"], Fo["output_size"], Fo["N"] * Fo["step_ratio"])
    check(WORST, "fold_mod", "Folding forward", out, r32["outs"][0], r64["outs"][0], F_FWD)
    force = _masks("fold", mod.decisions["pre"], r32["dec"], r64["dec"])
    first = _grads_check("fold", "fold", mod, [xg, gg], [out], force, "fold_mod")
    del mod.decisions
    again = _grads_check("fold", "fold", mod, [xg, gg], [mod(xg, gg)], force, "fold_mod")
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_folding_forward_memory(V, dev):
    """One Folding forward at B 2, N 256, C 64, G 1024, r 2, output 256 allocates less than one
    [B, G + C + 2, N r] float tensor (U plus the output are about a third of it)."""
    from models import vrcnet as M
    B, N, C, G, r, Co = 2, 256, 64, 1024, 2, 256
    torch.manual_seed(1)
    mod = M.Folding(C, Co, r, G).to(dev)
    rows = torch.randn(B * N, C, device=dev, requires_grad=True)
    g = torch.randn(B, G, device=dev, requires_grad=True)
    mod.forward_rows(rows, g)                                            # warm the allocator's pools and the library
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = mod.forward_rows(rows, g)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    print(f"Folding forward: {delta} bytes of new memory; one [B, G + C + 2, N r] float tensor is {B * (G + C + 2) * N * r * 4}")
    assert y.shape == (B * N * r, Co)
    assert delta < B * (G + C + 2) * N * r * 4


def _enc_force(what, rec, d32, d64, cfg, B):
    """The encoder inside the decoder, as tests/test_vrc_gpu.py checks it alone: geometry exact, masks, pool
    slots and conv5 winners under the cap rule -> the encoder's force dict."""
    for lv in range(4):
        for i in range(len(cfg["knn_list"])):
            assert torch.equal(rec["knn"][lv][i].cpu().long(), d64.idx[f"knn{lv + 1}.{i}"]), (what, lv, i)
    for lv in (1, 2, 3):
        assert torch.equal(rec["fps"][lv - 1].cpu().long(), d64.idx[f"fps{lv}"]), (what, lv)
        assert torch.equal(rec["pn_idx"][lv - 1].cpu().long(), d64.idx[f"pn_idx{lv}"]), (what, lv)
    for i, lv in enumerate((2, 1, 0)):
        assert torch.equal(rec["three_nn"][i].cpu().long(), d64.idx[f"three_nn{lv}"]), (what, lv)
    force = {}
    for name in d64.mask:
        t = rec["pre"][name].detach()
        ref = d64.pre[name]
        if t.dim() == 2 and ref.dim() == 2 and t.shape[1] != ref.shape[1]:
            t = t[:, :ref.shape[1]]                                      # '.P': only x1 | x2p pass a ReLU
        force[name] = _mask_check(what + " enc", t > 0, d32, d64, name)
    for lv in (1, 2, 3):
        force[f"slot{lv}"] = _slot_check(what + " enc", rec["slot"][lv - 1], d32, d64, f"slot{lv}", f"x{lv}")
    n4 = cfg["pts_num"][3]
    win = rec["win"].cpu().long() - torch.arange(B).view(B, 1) * n4
    assert bool(((win >= 0) & (win < n4)).all())
    force["win"] = _slot_check(what + " enc", win, d32, d64, "win", "conv5")
    return force


@pytest.mark.parametrize("name", ["dec_fold", "dec_ef"])
def test_decoder_against_the_restatement(V, dev, refs, name):
    r64, r32 = refs[name, torch.float64], refs[name, torch.float32]
    d64, d32 = r64["dec"], r32["dec"]
    cfg = D.DECS[name]
    B = cfg["B"]
    Pr, (g, pin), _ = D.fixture(name)
    mod = _build(name, dev)
    assert all(torch.equal(v.cpu(), Pr[k]) for k, v in mod.state_dict().items())
    mod.decisions = {}
    gg, pg = g.to(dev).requires_grad_(True), pin.to(dev).requires_grad_(True)
    outs = mod(gg, pg)
    rec = mod.decisions
    for i, (o, label) in enumerate(zip(outs, ("coarse_raw", "coarse_high", "coarse", "fine"))):
        assert tuple(o.shape) == tuple(r64["outs"][i].shape), label
        check(WORST, "dec_fwd", f"{name} {label}", o, r32["outs"][i], r64["outs"][i], F_FWD)
    force = _masks(name, rec["pre"], d32, d64)
    force["enc"] = _enc_force(name, rec["enc"], d32.enc, d64.enc, cfg, B)
    for key in ("fps", "topk"):                                          # value-dependent decisions: exact
        assert torch.equal(rec[key].cpu().long(), d64.idx[key]), key
        force[key] = rec[key].cpu().long()
    tags = [t for t in ("exp1", "exp2") if t + ".knn" in d64.idx]
    assert tags == (["exp1", "exp2"] if name == "dec_ef" else [])
    for tag in tags:
        assert torch.equal(rec["knn"][tag].cpu().long(), d64.idx[tag + ".knn"]), tag
        force[tag + ".knn"] = rec["knn"][tag].cpu().long()
        force[tag + ".slot"] = _slot_check(name, rec["slot"][tag], d32, d64, tag + ".slot", tag + ".H")
    _grads_check(name, name, mod, [gg, pg], outs, force, "dec_bwd", none=("conv_s1.", "conv_s2.", "conv_s3."))


def _small_decoder(dev, num_fps, num_coarse, num_fine, folding):
    from models import vrcnet as M
    E = D.DEC_FOLD
    torch.manual_seed(5)
    mod = M.MSAP_SKN_decoder(E["num_coarse_raw"], num_fps, num_coarse, num_fine, E["layers"], E["knn_list"], E["pk"],
                             points_label=folding, local_folding=folding, pts_num=E["pts_num"]).to(dev).eval()
    g = R.make_features(5, E["B"], 1024, 1).squeeze(2).to(dev).requires_grad_(True)
    pin = R.make_points(5, E["B"], E["n"]).transpose(1, 2).contiguous().to(dev)
    mod.decisions = {}
    return mod, g, pin


def test_shortcut_num_fps_covers_every_point(V, dev):
    mod, g, pin = _small_decoder(dev, 64, 64, 128, True)                # 64 points: no FPS, no ranking
    raw, high, coarse, fine = mod(g, pin)
    rec = mod.decisions
    assert "fps" not in rec and "topk" not in rec
    assert torch.equal(rec["coarse_fps"], high.transpose(1, 2).reshape(-1, 3)), "coarse_fps is coarse_high"
    assert torch.equal(coarse, high) and tuple(fine.shape) == (2, 3, 128)
    dg, = torch.autograd.grad(fine.sum() + coarse.sum(), [g])
    assert bool(torch.isfinite(dg).all())


def test_shortcut_num_coarse_covers_the_sampled_points(V, dev):
    mod, g, pin = _small_decoder(dev, 32, 32, 64, True)                 # FPS to 32, then no ranking
    raw, high, coarse, fine = mod(g, pin)
    rec = mod.decisions
    assert "topk" not in rec and tuple(rec["fps"].shape) == (2, 32)
    want = torch.gather(high, 2, rec["fps"].long().unsqueeze(1).expand(-1, 3, -1))
    assert torch.equal(coarse, want) and tuple(fine.shape) == (2, 3, 64)


def test_shortcut_num_coarse_is_num_fine(V, dev):
    mod, g, pin = _small_decoder(dev, 32, 16, 16, False)
    raw, high, coarse, fine = mod(g, pin)
    assert tuple(coarse.shape) == (2, 3, 16) and torch.equal(fine, coarse), "fine is coarse"
    want = torch.gather(torch.gather(high, 2, mod.decisions["fps"].long().unsqueeze(1).expand(-1, 3, -1)), 2,
                        mod.decisions["topk"].long().unsqueeze(1).expand(-1, 3, -1))
    assert torch.equal(coarse, want)


def test_equal_scores_select_the_lower_index_first(V, dev):
    from models.vrcnet import rank_scores
    s = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0, 2.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]], device=dev)
    got = rank_scores(s, 4)
    assert got.dtype == torch.int32
    assert got.cpu().tolist() == [[1, 2, 4, 5], [0, 1, 2, 3]]
