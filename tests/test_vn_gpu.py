"""The Vector-Neuron kernels, modules and encoders on the GPU (csrc/vn.hip, ured_hip/vn.py,
network/VN/) against tests/vn_ref.py, which tests/test_vn_ref.py pins to tests/golden/vn.npz (the
reference's own modules in float64).

Tolerance, from tests/tol_check.py: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|, f = 1e-5
forward and running statistics, 2e-5 gradients; ref32 is the same restatement in float32 on the CPU.
Nothing is derived from the GPU's output. Neighbour indices, leaky masks and pool winners are compared
exactly, and every gradient of two runs bit for bit. The seeds come from the golden: for them
test_vn_ref.py asserts that every kernel-level decision, and every encoder-level kNN and pool-winner
decision, of the float64 restatement lies at least 1e-4 from a flip. At encoder level a few leaky
decisions in 10^5 lie closer: there the GPU's mask must equal the float64 mask wherever the float64
margin is at least 1e-4, forward values are compared with the restatement's own decisions (the
function is continuous across a mask flip), and gradients with the restatement evaluated under the
GPU's exported mask. The encoder's maximum over the N points is a third kind of winner (8184 per
batch, about 0.16 % of them within 1e-4 of the runner-up): it is exported and treated like the masks.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import vn_ref as R
from conftest import GOLDEN
from tol_check import F_FWD, F_GRAD, check

pytestmark = pytest.mark.gpu
WORST = {}
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "vn.npz")))


@pytest.fixture(scope="module")
def G(dev):
    from ured_hip import vn
    yield vn
    for fam, (ratio, what) in sorted(WORST.items()):
        print(f"worst ratio {fam:14s} {ratio:.3f}  ({what})")


@pytest.fixture(autouse=True)
def _vn_debug_word():
    """The debug build's bounds word of vn.hip (file id 15), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_vn"):
        return
    fn = mod._lib.ured_dbg_vn
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): vn.hip:{v & 0xFFFFFFFF}"


def _bitwise(a, b, what):
    assert torch.equal(a, b), f"{what}: two runs differ"


def _bn(kind, Co, inp, training, dev):
    bn = kind(Co).to(dev)
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"].float())
        bn.bias.copy_(inp["beta"].float())
        bn.running_mean.copy_(inp["rmean"].float())
        bn.running_var.copy_(inp["rvar"].float())
    bn.train(training)
    return bn


# ---------------- kernel level ----------------

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [5, 33, 130])
def test_knn_rows(G, dev, B, N):
    rng = np.random.default_rng(B * 1000 + N)
    for D in (3, 63, 126, 256):
        # a 1/8 grid, few distinct values per coordinate, duplicated points: exact distances, exact ties
        x = torch.from_numpy(rng.integers(0, 3 if D > 3 else 5, size=(B, N, D)).astype(np.float32) / 8)
        x[:, N - 1] = x[:, 0]
        x[:, N // 2] = x[:, 1]
        for K in (1, 4, 20, 32):
            if K > N:
                with pytest.raises(ValueError, match="exceeds the cloud"):
                    G.knn_rows(x.to(dev), K)
                continue
            got = G.knn_rows(x.to(dev), K)
            assert got.dtype == torch.int32 and tuple(got.shape) == (B, N, K)
            want, _ = R.knn_rows(x.double(), K)
            assert torch.equal(got.cpu().long(), want), f"B{B} N{N} D{D} K{K}"
            assert bool((got[:, 0, 0] == 0).all())           # the query itself, ahead of its duplicate N - 1


@pytest.mark.parametrize("ci", range(len(R.ACT_CASES)))
def test_act_kernel(G, dev, gold, ci):
    case = R.ACT_CASES[ci]
    B, C, Co, N, k, shared, pool, training, edge, special = case
    inp = R.act_case_inputs(case, int(gold["act_seeds"][ci]))
    r64 = R.act_run(case, inp, F64)
    r32 = R.act_run(case, inp, F32, mask=r64["mask"])
    tag = f"{'edge' if edge else 'point'} B{B} C{C} Co{Co} N{N} k{k} {'shared' if shared else 'perch'} {pool} " \
          f"{'train' if training else 'eval'} {special or ''}"
    runs = []
    for _ in range(2):
        bn = _bn(torch.nn.BatchNorm2d if edge else torch.nn.BatchNorm1d, Co, inp, training, dev)
        x, Wf, Wd = (inp[n].float().to(dev).requires_grad_(True) for n in ("x", "Wf", "Wd"))
        if edge:
            out, mask = G.vn_edge(x, inp["idx"].to(dev), Wf, Wd, bn, pool)
        else:
            out, mask = G.vn_point(x, Wf, Wd, bn)
        out.backward(inp["g"].float().to(dev).view(out.shape))
        runs.append((out.detach(), mask, x.grad, Wf.grad, Wd.grad, bn.weight.grad, bn.bias.grad, bn))
    out, mask, gx, gWf, gWd, gg, gb, bn = runs[0]
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == ((B, N, k, Co) if edge else (B, N, Co))
    assert torch.equal(mask.cpu().bool().view(B, N, k, Co), r64["mask"]), f"{tag}: leaky masks"
    want_shape = (B, N, 3, Co) if pool == "mean" else (B, N, k, 3, Co)
    assert tuple(out.shape) == want_shape
    check(WORST, "act fwd", tag, out, r32["out"].view(want_shape), r64["out"].view(want_shape), F_FWD)
    check(WORST, "act stats", tag + " running_mean", bn.running_mean, r32["running_mean"], r64["running_mean"], F_FWD)
    check(WORST, "act stats", tag + " running_var", bn.running_var, r32["running_var"], r64["running_var"], F_FWD)
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    for i, (name, got) in enumerate((("gx", gx), ("gWf", gWf), ("gWd", gWd), ("ggamma", gg), ("gbeta", gb))):
        check(WORST, "act grad", f"{tag} {name}", got, r32[name], r64[name], F_GRAD)
        _bitwise(got, runs[1][2 + i], f"{tag} {name}")
    if special == "origin":                                  # p = 0 exactly at edge (2, 0): a zero output
        assert pool == "none" and bool((out[:, 2, 0] == 0).all()) and bool((mask[:, 2, 0] == 1).all())
        assert bool(torch.isfinite(gx).all())
        # that edge's gradient is of order nb / 1e-6 and sets max|ref64| above: the other points again, alone
        rest = [n for n in range(N) if n != 2]
        check(WORST, "act grad", f"{tag} gx without the origin", gx[:, rest], r32["gx"][:, rest], r64["gx"][:, rest], F_GRAD)


@pytest.mark.parametrize("ci", range(len(R.POOL_CASES)))
def test_maxpool_kernel(G, dev, gold, ci):
    N, k, C = R.POOL_CASES[ci]
    x64, Wp, g = R.pool_case_inputs(R.POOL_CASES[ci], int(gold["pool_seeds"][ci]))
    refs = []
    slot64 = None
    for dt in (F64, F32):
        xs = x64.to(dt).clone().requires_grad_(True)
        out, win, _ = R.maxpool(xs, Wp.to(dt), slot64)
        slot64 = win
        out.backward(g.to(dt))
        refs.append((out.detach(), xs.grad))
    runs = []
    for _ in range(2):
        x = x64.float().to(dev).requires_grad_(True)
        wp = Wp.float().to(dev).requires_grad_(True)
        out, slot = G.VnMaxPoolFn.apply(x, wp)
        out.backward(g.float().to(dev))
        assert wp.grad is None                               # as in the reference
        runs.append((out.detach(), slot, x.grad))
    out, slot, gx = runs[0]
    tag = f"N{N} k{k} C{C}"
    assert slot.dtype == torch.uint8 and torch.equal(slot.cpu().long(), slot64), f"{tag}: winners"
    assert torch.equal(out.cpu(), refs[1][0]), f"{tag}: the forward is not a copy of the winning edge"
    check(WORST, "maxpool grad", tag, gx, refs[1][1], refs[0][1], F_GRAD)
    _bitwise(gx, runs[1][2], tag + " grad")


def test_maxpool_exact_tie(G, dev):
    """Edges 1 and 3 are copies of each other and beat the rest: <x,d> ties exactly, the lowest j wins."""
    B, N, k, C = 1, 3, 4, 5
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (B, N, k, 3, C), generator=g).float() / 8
    Wp = torch.eye(C)                                        # d = x: <x,d> = |x|^2, exact on the grid
    x[:, :, 1] = 2.0
    x[:, :, 3] = 2.0
    out, slot = G.VnMaxPoolFn.apply(x.to(dev), Wp.to(dev))
    assert bool((slot == 1).all()) and bool((out == 2.0).all())


@pytest.mark.parametrize("C", [1, 170, 682])
def test_frame(G, dev, C):
    B, N = 2, 33
    g = torch.Generator().manual_seed(C)
    x64, z64 = torch.randn(B, N, 3, C, generator=g, dtype=F64), torch.randn(B, N, 3, 3, generator=g, dtype=F64)
    go = torch.randn(B, N, 3, C, generator=g, dtype=F64)
    refs = []
    for dt in (F64, F32):
        xs, zs = x64.to(dt).clone().requires_grad_(True), z64.to(dt).clone().requires_grad_(True)
        o = R.frame(xs, zs)
        o.backward(go.to(dt))
        refs.append((o.detach(), xs.grad, zs.grad))
    runs = []
    for _ in range(2):
        x, z = x64.float().to(dev).requires_grad_(True), z64.float().to(dev).requires_grad_(True)
        o = G.VnFrameFn.apply(x, z)
        o.backward(go.float().to(dev))
        runs.append((o.detach(), x.grad, z.grad))
    for i, (name, f) in enumerate((("out", F_FWD), ("gx", F_GRAD), ("gz", F_GRAD))):
        check(WORST, "frame", f"C{C} {name}", runs[0][i], refs[1][i], refs[0][i], f)
        _bitwise(runs[0][i], runs[1][i], f"frame C{C} {name}")


# ---------------- encoder level ----------------

def _gpu_decisions(dec):
    return ([i.cpu().long() for i in dec["idx"]], [m.cpu().bool() for m in dec["masks"]],
            [s.cpu().long() for s in dec["slots"]])


@pytest.mark.parametrize("pooling", ["mean", "max"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_encoder(G, dev, gold, pooling, mode):
    from network.VN.vn_encoder import vn_encoder
    from network.VN.vn_retrieval import vn_retrieval
    seed = int(gold[f"{pooling}_{mode}_seed"])
    training = mode == "train"
    B, N, L = R.ENC["B"], R.ENC["N"], R.ENC["latent"]
    P, x = R.encoder_params(seed, pooling), R.encoder_input(seed)
    with torch.no_grad():
        r64 = R.encoder(P, x, training, pooling)
        r32 = R.encoder(R.cast(P, F32), x.float(), training, pooling, idx=r64["idx"], masks=r64["masks"],
                        slots=r64["slots"] or None)
    cfg = dict(n_knn=R.ENC["n_knn"], pooling=pooling, target_latent_dim=L)
    net = vn_encoder(cfg).to(dev)
    net.load_state_dict(R.cast(P, F32), strict=True)          # the reference's keys
    net.train(training)
    net.decisions = {}
    xg = x.float().to(dev)
    if training:
        gf, pf = net(xg)
    else:
        with torch.no_grad():
            gf, pf = net(xg)
    idx, masks, slots = _gpu_decisions(net.decisions)
    tag = f"{pooling} {mode}"
    assert tuple(gf.shape) == (B, L) and tuple(pf.shape) == (B, L, N)
    assert len(idx) == 4 and len(masks) == 7 and len(slots) == (4 if pooling == "max" else 0)
    for li in range(4):
        assert torch.equal(idx[li], r64["idx"][li]), f"{tag}: neighbours of level {li + 1}"
        if pooling == "max":
            assert torch.equal(slots[li], r64["slots"][li]), f"{tag}: pool winners of level {li + 1}"
    for li in range(7):
        m64, mg = r64["masks"][li], r64["mask_margins"][li]
        sure = mg >= R.MARGIN
        assert torch.equal(masks[li].view(m64.shape)[sure], m64[sure]), f"{tag}: leaky mask of layer {li + 1}"
    # the maximum over the N points, 3 * 682 winners per cloud: as for the masks, a few lie within 1e-4
    npool = net.decisions["npool"].cpu()
    sure = r64["npool_margin"] >= R.MARGIN
    flips = int((npool != r64["npool"]).sum())
    print(f"{tag}: {flips} of {npool.numel()} winners of the max over N differ from float64's ({int((~sure).sum())} within 1e-4)")
    assert torch.equal(npool[sure], r64["npool"][sure]), f"{tag}: winners of the max over N"
    check(WORST, "encoder", f"{tag} global_f vs golden", gf, r32["global_f"], gold[f"{pooling}_{mode}_global"], F_FWD)
    check(WORST, "encoder", f"{tag} point_feat[::4] vs golden", pf[:, :, ::4], r32["point_feat"][:, :, ::4],
          gold[f"{pooling}_{mode}_point_sub"], F_FWD)
    check(WORST, "encoder", f"{tag} point_feat", pf, r32["point_feat"], r64["point_feat"], F_FWD)
    sd = net.state_dict()
    for k in sorted(r64["stats"]):
        check(WORST, "encoder", f"{tag} {k}", sd[k], r32["stats"][k], r64["stats"][k], F_FWD)
    ret = vn_retrieval(cfg).to(dev)
    ret.load_state_dict({k: v for k, v in R.cast(P, F32).items() if not k.startswith("per_point_f")}, strict=True)
    ret.train(training)
    with torch.set_grad_enabled(training):
        check(WORST, "encoder", f"{tag} vn_retrieval", ret(xg), r32["global_f"], gold[f"ret_{pooling}_{mode}_global"], F_FWD)
    if not training:
        return
    # gradients: the restatement under the GPU's own decisions
    masks_r = [m.view(r64["masks"][i].shape) for i, m in enumerate(masks)]
    _, g64 = R.encoder_grads(P, x, pooling, seed, F64, idx=idx, masks=masks_r, slots=slots or None, npool=npool)
    _, g32 = R.encoder_grads(P, x, pooling, seed, F32, idx=idx, masks=masks_r, slots=slots or None, npool=npool)
    g1, g2 = (t.float().to(dev) for t in R.encoder_cotangents(seed))
    grads = []
    for run in range(2):
        if run:
            net.zero_grad(set_to_none=True)
            net.decisions = None
            gf, pf = net(xg)
        ((gf * g1).sum() + (pf * g2).sum()).backward()
        grads.append({k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()})
    scale = g64["linear1.weight"].abs().max().item()
    missed = []                                              # every parameter is measured before the test fails
    for k, p in net.named_parameters():
        if k.startswith("pool"):
            assert grads[0][k] is None, f"{tag}: {k} takes no gradient in the reference"
            continue
        assert grads[0][k] is not None, f"{tag}: no gradient of {k}"
        if k == "linear1.bias":
            # a bias before a training-mode BatchNorm: the gradient is 0 in exact arithmetic and all three
            # computations hold rounding residue, so the floor is taken from the scale of its layer's
            # weight gradient (the same upstream values, times inputs of order 1)
            assert float(grads[0][k].abs().max()) <= 3 * float(g32[k].abs().max()) + F_GRAD * scale, f"{tag}: {k}"
        else:
            try:
                check(WORST, "encoder grad", f"{tag} {k}", grads[0][k], g32[k], g64[k], F_GRAD)
            except AssertionError as e:
                missed.append(str(e))
        _bitwise(grads[0][k], grads[1][k], f"{tag} gradient of {k}")
    assert not missed, "\n".join(missed)


def test_module_layouts(G, dev):
    """forward() of the layer modules takes the reference's [B, C, 3, N, k] layout."""
    from network.VN import vn_layers as L
    from network.VN.vn_dgcnn_util import get_graph_feature, knn
    torch.manual_seed(0)
    B, C, N, k = 2, 3, 16, 4
    x = torch.randn(B, C, 3, N, device=dev)
    idx = knn(x.view(B, -1, N), k)
    assert idx.dtype == torch.long and tuple(idx.shape) == (B, N, k)
    want, _ = R.knn_rows(x.cpu().double().permute(0, 3, 2, 1).reshape(B, N, 3 * C), k)
    assert torch.equal(idx.cpu(), want)
    e = get_graph_feature(x, k=k)
    assert tuple(e.shape) == (B, 2 * C, 3, N, k)
    layer = L.VNLinearLeakyReLU(2 * C, 5).to(dev)
    y = layer(e)                                             # dim = 5: the BatchNorm over all B * N * k edges
    assert tuple(y.shape) == (B, 5, 3, N, k)
    rows = x.permute(0, 3, 2, 1).contiguous()
    fused = layer.forward_graph(rows, idx.int(), "none")     # [B, N, k, 3, 5]
    # the per-edge product and the two per-point products round differently; both are the same function
    assert float((fused.permute(0, 4, 3, 1, 2) - y).abs().max()) <= 1e-4 * float(y.abs().max())
    pool = L.VNMaxPool(5).to(dev)
    assert tuple(pool(y).shape) == (B, 5, 3, N)
    std, z = L.VNStdFeature(8).to(dev)(torch.randn(B, 8, 3, N, device=dev))
    assert tuple(std.shape) == (B, 8, 3, N) and tuple(z.shape) == (B, 3, 3, N)


def test_edge_layer_memory(G, dev):
    """One mean-pooled edge layer at B 2, N 256, k 16, C 21 -> 21: the forward, with its outputs and
    what it keeps for the backward alive, must allocate less than one [B,N,k,3,Co] fp32 tensor (2.06 MB)."""
    B, N, k, C, Co = 2, 256, 16, 21, 21
    torch.manual_seed(0)
    x = torch.randn(B, N, 3, C, device=dev, requires_grad=True)
    idx = G.knn_rows(x.detach().view(B, N, 3 * C), k)
    Wf = torch.randn(Co, 2 * C, device=dev, requires_grad=True)
    Wd = torch.randn(Co, 2 * C, device=dev, requires_grad=True)
    bn = torch.nn.BatchNorm2d(Co).to(dev)
    out, mask = G.vn_edge(x, idx, Wf, Wd, bn, "mean")          # warm-up: code objects, allocator pools
    out.sum().backward()
    del out, mask
    x.grad = Wf.grad = Wd.grad = None
    bn.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, mask = G.vn_edge(x, idx, Wf, Wd, bn, "mean")
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    big = B * N * k * 3 * Co * 4
    print(f"edge layer forward: peak delta {delta / 1e6:.2f} MB; one per-edge tensor {big / 1e6:.2f} MB")
    assert tuple(out.shape) == (B, N, 3, Co) and big == 2064384
    assert delta < big
