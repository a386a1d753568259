"""3D-GCN on the GPU (csrc/gcn.hip, ured_hip/gcn.py, network/P_3DGC.py, network/gc3d_encoder.py)
against tests/gcn_ref.py and tests/golden/gcn.npz (the reference's own modules in float64).

Tolerance, from tests/tol_check.py: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|, f = 1e-5
forward and 2e-5 gradients; ref32 is the same restatement in float32 on the CPU. Nothing is derived
from the GPU's output. Indices and winning slots are compared exactly, the pooling forward bit for
bit (a max of copies), and every gradient of two runs bit for bit. tests/test_gcn_ref.py asserts, for
the reference alone, that no ReLU / max / nearest-neighbour decision of these inputs lies within
rounding of a flip (kernel cases: every theta and product is exact in fp32).

Of the encoder's per-point features the golden holds every 16th point (the file's size limit); the
whole tensor is compared with gcn_ref.encoder in float64, which test_gcn_ref.py pins to the golden.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import gcn_ref as R
from conftest import GOLDEN
from tol_check import F_FWD, F_GRAD, check

pytestmark = pytest.mark.gpu
WORST = {}
MOD = dict(B=2, V=64, n=4, S=3, cin=4, cout=8)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "gcn.npz")))


@pytest.fixture(scope="module")
def G(dev):
    from ured_hip import gcn
    yield gcn
    for fam, (ratio, what) in sorted(WORST.items()):
        print(f"worst ratio {fam:14s} {ratio:.3f}  ({what})")


@pytest.fixture(autouse=True)
def _gcn_debug_word():
    """The debug build's bounds word of gcn.hip (file id 14), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_gcn"):
        return
    fn = mod._lib.ured_dbg_gcn
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): gcn.hip:{v & 0xFFFFFFFF}"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _f(t):
    return None if t is None else t.float()


def _bitwise(a, b, what):
    assert torch.equal(a, b), f"{what}: two runs differ"


# ---------------- kernel level ----------------

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [5, 33, 130])
def test_neighbor_dirs(G, dev, B, V):
    rng = np.random.default_rng(B * 1000 + V)
    for n in (1, 4, 10):
        v = _t(rng.random((B, V, 3), dtype=np.float32))
        idx = _t(rng.integers(0, V, size=(B, V, n)).astype(np.int32))
        idx[:, 2, 0] = 2                                   # a coincident neighbour: the vertex itself
        v[:, 4] = v[:, 3]                                  # ... and a duplicate of another vertex
        idx[:, 3, n - 1] = 4
        got = G.neighbor_dirs(v.to(dev), idx.to(dev))
        assert tuple(got.shape) == (B, V, n, 3) and got.dtype == torch.float32
        check(WORST, "dirs", f"B{B} V{V} n{n}", got, R.dirs(v, idx), R.dirs(v.double(), idx), F_FWD)
        assert bool((got[:, 2, 0] == 0).all()) and bool((got[:, 3, n - 1] == 0).all())


@pytest.mark.parametrize("ci", range(len(R.KERNEL_CASES)))
@pytest.mark.parametrize("layer", [False, True], ids=["surface", "layer"])
def test_conv_kernel(G, dev, gold, ci, layer):
    case = R.KERNEL_CASES[ci]
    B, V, n, S, C = case
    dirn, sdn, feat, idx, g = R.kernel_case(case, int(gold["kern_seeds"][ci, int(layer)]), layer)
    out64, slot64 = R.conv_fwd(dirn, sdn, feat, idx, S)
    gf64, gs64 = R.conv_bwd(g, dirn, sdn, feat, idx, slot64, S)
    out32, slot32 = R.conv_fwd(_f(dirn), _f(sdn), _f(feat), idx, S)
    gf32, gs32 = R.conv_bwd(_f(g), _f(dirn), _f(sdn), _f(feat), idx, slot32, S)
    tag = f"{'layer' if layer else 'surface'} B{B} V{V} n{n} S{S} C{C}"
    runs = []
    for _ in range(2):
        sd = _f(sdn).to(dev).requires_grad_(True)
        ft = None if feat is None else _f(feat).to(dev).requires_grad_(True)
        out, slot = G.GcnConvFn.apply(_f(dirn).to(dev), sd, ft, idx.to(dev), S)
        out.backward(_f(g).to(dev))
        runs.append((out.detach(), slot, sd.grad, None if ft is None else ft.grad))
    out, slot, gs, gf = runs[0]
    assert slot.dtype == torch.uint8 and tuple(slot.shape) == (B * V, S, C)
    assert torch.equal(slot.cpu().long(), slot64), f"{tag}: winning slots"
    check(WORST, "conv fwd", tag, out, out32, out64, F_FWD)
    check(WORST, "conv grad_sdn", tag, gs, gs32, gs64, F_GRAD)
    if layer:
        check(WORST, "conv grad_feat", tag, gf, gf32, gf64, F_GRAD)
        _bitwise(gf, runs[1][3], tag + " grad_feat")
    _bitwise(gs, runs[1][2], tag + " grad_sdn")
    # vertex 0 has every theta == 0: its maxima are an exact 0, won by slot 0
    assert bool((slot.view(B, V, S, C)[:, 0] == 0).all())
    if not layer:
        assert bool((out.view(B, V, C)[:, 0] == 0).all())


@pytest.mark.parametrize("V", [5, 33, 130])
@pytest.mark.parametrize("C", [1, 8, 100, 128])
def test_pool_kernel(G, dev, V, C):
    B = 2
    rng = np.random.default_rng(V * 1000 + C)
    for k in (1, 4):
        for P in sorted({1, V // 4}):
            feat = _t(rng.standard_normal((B * V, C)).astype(np.float32))
            feat[1] = feat[0]                              # equal rows: ties, the lowest slot wins
            idx = _t(rng.integers(0, V, size=(B, V, k)).astype(np.int32))
            sample = _t(rng.integers(0, V, size=(P,)).astype(np.int32))
            if P > 1:
                sample[P - 1] = sample[0]                  # a repeated entry
            g = _t(rng.standard_normal((B * P, C)).astype(np.float32))
            want, wslot = R.pool_fwd(feat, idx, sample)
            g64 = R.pool_bwd(g.double(), idx, sample, wslot, V)
            g32 = R.pool_bwd(g, idx, sample, wslot, V)
            tag = f"V{V} C{C} k{k} P{P}"
            runs = []
            for _ in range(2):
                x = feat.to(dev).requires_grad_(True)
                out, slot = G.GcnPoolFn.apply(x, idx.to(dev), sample.to(dev))
                out.backward(g.to(dev))
                runs.append((out.detach(), slot, x.grad))
            out, slot, gx = runs[0]
            assert torch.equal(out.cpu(), want), f"{tag}: forward is not bitwise the max of copies"
            assert torch.equal(slot.cpu().long(), wslot), f"{tag}: winning slots"
            check(WORST, "pool grad", tag, gx, g32, g64, F_GRAD)
            _bitwise(gx, runs[1][2], tag + " grad")


@pytest.mark.parametrize("M,K,N", [(66, 4, 32), (130, 128, 1024), (66, 128, 32), (130, 4, 1024)])
def test_linear(G, dev, M, K, N):
    rng = np.random.default_rng(M + K + N)
    x, w, b, g = (_t(rng.standard_normal(s)) for s in ((M, K), (K, N), (N,), (M, N)))
    refs = []
    for dt in (torch.float32, torch.float64):
        xs, ws, bs = (t.to(dt).clone().requires_grad_(True) for t in (x, w, b))
        y = xs @ ws + bs
        y.backward(g.to(dt))
        refs.append((y.detach(), xs.grad, ws.grad, bs.grad))
    xs, ws, bs = (t.float().to(dev).requires_grad_(True) for t in (x, w, b))
    y = G.GcnLinearFn.apply(xs, ws, bs)
    y.backward(g.float().to(dev))
    tag = f"M{M} K{K} N{N}"
    check(WORST, "linear", tag + " out", y, refs[0][0], refs[1][0], F_FWD)
    for name, got, i in (("dx", xs.grad, 1), ("dw", ws.grad, 2), ("db", bs.grad, 3)):
        check(WORST, "linear", f"{tag} {name}", got, refs[0][i], refs[1][i], F_GRAD)


# ---------------- module level ----------------

def test_indices_vs_golden(G, dev, gold):
    import network.P_3DGC as M
    v = _t(gold["mod_vertices"]).float().to(dev)
    idx = M.get_neighbor_index(v, MOD["n"])
    assert idx.dtype == torch.long
    np.testing.assert_array_equal(idx.cpu().numpy(), gold["mod_idx"])
    near = M.get_nearest_index(v, _t(gold["mod_pool_v"]).float().to(dev))
    assert near.dtype == torch.long and tuple(near.shape) == (2, 64, 1)
    np.testing.assert_array_equal(near.cpu().numpy(), gold["mod_nearest"])
    d = M.get_neighbor_direction_norm(v, idx)
    ref = R.dirs(_t(gold["mod_vertices"]), idx.cpu())
    check(WORST, "modules", "get_neighbor_direction_norm", d, R.dirs(v.cpu(), idx.cpu()), ref, F_FWD)
    got = M.indexing_neighbor(v, idx)
    assert torch.equal(got.cpu(), v.cpu()[torch.arange(2).view(2, 1, 1), idx.cpu()])


def test_conv_surface_vs_golden(G, dev, gold):
    import network.P_3DGC as M
    v64, idx = _t(gold["mod_vertices"]), _t(gold["mod_idx"]).long()
    d32 = _t(gold["mod_surf.directions"]).float().requires_grad_(True)
    y32 = R.conv_surface(d32, MOD["S"], idx, v64.float())
    y32.backward(_t(gold["mod_g"]).float())
    mod = M.Conv_surface(MOD["cout"], MOD["S"]).to(dev)
    mod.load_state_dict({"directions": _t(gold["mod_surf.directions"]).float()}, strict=True)
    y = mod(idx.to(dev), v64.float().to(dev))
    y.backward(_t(gold["mod_g"]).float().to(dev))
    check(WORST, "modules", "Conv_surface out", y, y32, gold["mod_surf_out"], F_FWD)
    check(WORST, "modules", "Conv_surface grad directions", mod.directions.grad, d32.grad, gold["mod_surf_gdir"], F_GRAD)


def test_conv_layer_vs_golden(G, dev, gold):
    import network.P_3DGC as M
    v64, idx = _t(gold["mod_vertices"]), _t(gold["mod_idx"]).long()
    w, b, d = (_t(gold["mod_layer." + k]).float().requires_grad_(True) for k in ("weights", "bias", "directions"))
    x32 = _t(gold["mod_fmap"]).float().requires_grad_(True)
    y32 = R.conv_layer(w, b, d, MOD["S"], idx, v64.float(), x32)
    y32.backward(_t(gold["mod_g"]).float())
    mod = M.Conv_layer(MOD["cin"], MOD["cout"], MOD["S"]).to(dev)
    mod.load_state_dict({k: _t(gold["mod_layer." + k]).float() for k in ("weights", "bias", "directions")}, strict=True)
    x = _t(gold["mod_fmap"]).float().to(dev).requires_grad_(True)
    y = mod(idx.to(dev), v64.float().to(dev), x)
    y.backward(_t(gold["mod_g"]).float().to(dev))
    check(WORST, "modules", "Conv_layer out", y, y32, gold["mod_layer_out"], F_FWD)
    for name, got, r32, key in (("weights", mod.weights.grad, w.grad, "gw"), ("bias", mod.bias.grad, b.grad, "gb"),
                                ("directions", mod.directions.grad, d.grad, "gdir"), ("feature_map", x.grad, x32.grad, "gx")):
        check(WORST, "modules", f"Conv_layer grad {name}", got, r32, gold["mod_layer_" + key], F_GRAD)


def test_pool_layer_vs_golden(G, dev, gold):
    import network.P_3DGC as M
    v64 = _t(gold["mod_vertices"])
    sample = _t(gold["mod_pool_sample"]).long()
    x32 = _t(gold["mod_pmap"]).float().requires_grad_(True)
    _, f32 = R.pool_layer(v64.float(), x32, sample)
    f32.backward(_t(gold["mod_gp"]).float())
    x = _t(gold["mod_pmap"]).float().to(dev).requires_grad_(True)
    torch.manual_seed(int(gold["mod_pool_seed"]))
    vp, fp = M.Pool_layer(4, 4)(v64.float().to(dev), x)
    fp.backward(_t(gold["mod_gp"]).float().to(dev))
    assert torch.equal(vp.cpu(), v64.float()[:, sample])
    check(WORST, "modules", "Pool_layer out", fp, f32, gold["mod_pool_out"], F_FWD)
    check(WORST, "modules", "Pool_layer grad feature_map", x.grad, x32.grad, gold["mod_pool_gx"], F_GRAD)


# ---------------- encoder level ----------------

@pytest.fixture(scope="module")
def enc_refs(gold):
    """gcn_ref.encoder in float64 and float32 per (V, mode), computed once."""
    out = {}
    for V in (128, 256):
        verts = _t(gold[f"enc{V}_vertices"])
        _, rseed, wseed = (int(s) for s in gold[f"enc{V}_seeds"])
        samples = R.encoder_samples(V, rseed)
        P = R.encoder_params(wseed)
        for mode in ("train", "eval"):
            with torch.no_grad():
                out[V, mode] = (R.encoder(R.cast(P, torch.float32), verts.float(), mode == "train", samples),
                                R.encoder(P, verts, mode == "train", samples))
    return out


@pytest.mark.parametrize("V", [128, 256])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_encoder_vs_golden(G, dev, gold, enc_refs, V, mode):
    from network.gc3d_encoder import GCN3D_ENCODER
    verts = _t(gold[f"enc{V}_vertices"]).float().to(dev)
    _, rseed, wseed = (int(s) for s in gold[f"enc{V}_seeds"])
    net = GCN3D_ENCODER().to(dev)
    net.load_state_dict(R.cast(R.encoder_params(wseed), torch.float32), strict=True)   # the reference's keys
    net.train(mode == "train")
    (fg32, feat32, st32), (fg64, feat64, st64) = enc_refs[V, mode]
    torch.manual_seed(rseed)
    if mode == "eval":
        with torch.no_grad():
            fg, feat = net(verts)
    else:
        fg, feat = net(verts)
    assert tuple(fg.shape) == (2, 256) and tuple(feat.shape) == (2, 256, V)
    tag = f"V{V} {mode}"
    check(WORST, "encoder", f"{tag} f_global vs golden", fg, fg32, gold[f"enc{V}_{mode}_fglobal"], F_FWD)
    check(WORST, "encoder", f"{tag} feat[::16] vs golden", feat[:, :, ::16], feat32[:, :, ::16],
          gold[f"enc{V}_{mode}_feat_sub"], F_FWD)
    check(WORST, "encoder", f"{tag} feat", feat, feat32, feat64, F_FWD)
    sd = net.state_dict()
    for k in sorted(st64):
        want = gold[f"enc{V}_train_{k}"] if mode == "train" else st64[k]
        check(WORST, "encoder", f"{tag} {k}", sd[k], st32[k], want, F_FWD)
    if mode == "eval":
        return
    grads = []
    for run in range(2):
        if run:
            net.zero_grad(set_to_none=True)
            torch.manual_seed(rseed)
            fg, feat = net(verts)
        (feat.sum() + fg.sum()).backward()
        grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{tag}: gradient of {k}"
        _bitwise(grads[0][k], grads[1][k], f"{tag} gradient of {k}")


def test_conv_layer_memory(G, dev):
    """B 2, V 512, n 10, S 7, C 128: the [B,V,n,S*C] tensor that the reference builds (three times over)
    is 36.7 MB; one fused Conv_layer forward + backward must stay below half of one of them."""
    import network.P_3DGC as M
    B, V, n, S, C = 2, 512, 10, 7, 128
    torch.manual_seed(0)
    v = torch.rand(B, V, 3, device=dev)
    idx = M.get_neighbor_index(v, n)
    dirn = M.get_neighbor_direction_norm(v, idx)
    mod = M.Conv_layer(C, C, S).to(dev)
    x = torch.randn(B, V, C, device=dev, requires_grad=True)
    g = torch.randn(B, V, C, device=dev)
    mod(idx, v, x, dirn).backward(g)                       # warm-up: code objects, allocator pools
    mod.zero_grad(set_to_none=True)
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    mod(idx, v, x, dirn).backward(g)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    big = B * V * n * S * C * 4
    print(f"Conv_layer forward + backward: peak delta {delta / 1e6:.2f} MB; the reference's tensor {big / 1e6:.2f} MB")
    assert delta < big / 2
