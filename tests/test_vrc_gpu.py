"""VRCNet's self-attention encoder on the GPU (csrc/vrc.hip, ured_hip/vrc.py, models/vrcnet.py) against
tests/vrc_ref.py in float64, which tests/test_vrc_ref.py pins to the reference's own modules.

Tolerance, from tests/tol_check.py: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|, f = 1e-5
forward and 2e-5 gradients; ref32 is the same restatement in float32 on the CPU. Nothing is derived
from the GPU's output. Decisions as in tests/test_pcn_gpu.py: kNN / FPS / three-NN indices are compared
exactly; a GPU ReLU mask, pool slot or max winner may differ from float64's own only where the deciding
value lies within the layer's forward tolerance of a flip (twice that for a slot or winner) and in at
most MASK_CAP (0.05 %) of a layer's elements; the float64 backward runs with the GPU's decisions forced
under fixed random cotangents, and every input and parameter gradient is compared as a whole tensor.
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import vrc_ref as R
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


def _eighths(rng, shape, lo=-16, hi=17):
    return torch.from_numpy(rng.integers(lo, hi, size=shape).astype(np.float64) / 8)


def _normal(rng, shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) * scale


def _tol(a32, a64, f=F_FWD):
    return FLOOR_MULT * (a32.double() - a64).abs().max().item() + f * a64.abs().max().item()


def _mask_check(what, got, d32, d64, name, mult=1.0):
    """The GPU's mask against float64's: equal wherever float64's pre-activation is at least the layer's
    forward tolerance from zero, and different in at most MASK_CAP of the layer."""
    pre64 = d64.pre[name]
    got = got.cpu().reshape(pre64.shape)
    tol = mult * _tol(d32.pre[name], pre64)
    diff = got != d64.mask[name]
    far = diff & (pre64.abs() >= tol)
    assert not bool(far.any()), f"{what} {name}: {int(far.sum())} masks differ beyond the forward tolerance {tol:.3e}"
    assert int(diff.sum()) <= MASK_CAP * diff.numel(), f"{what} {name}: {int(diff.sum())} of {diff.numel()} masks differ"
    return got


# ---------------- SaFn ----------------

def _sa_idx(rng, B, N, k):
    """Duplicates inside a row, a hub every row names, a point no row names, one index out of range."""
    idx = torch.from_numpy(rng.integers(0, N, size=(B, N, k))).int()
    idx[:, :, 0] = 0                                   # the hub
    if k >= 3:
        idx[:, :, 2] = idx[:, :, 1]                    # a duplicate inside every row
    if N > 1:
        idx[idx == N - 1] = 0                          # no row names the last point
    if k >= 2:
        idx[0, 0, k - 1] = N                           # out of range: a zero row, no gradient
    return idx


SA_CASES = [(1, 1, 1, 1, 8, 8), (1, 5, 5, 3, 24, 8), (2, 65, 10, 4, 16, 8), (3, 130, 20, 8, 32, 8), (1, 33, 32, 32, 128, 8)]


@pytest.mark.parametrize("B,N,k,rel,mid,share", SA_CASES)
def test_sa_core(V, dev, B, N, k, rel, mid, share):
    rng = np.random.default_rng(B * 1000 + N)
    ms = mid // share
    L, T = rel * (k + 1), k * ms
    P = _normal(rng, (B * N, 2 * rel + mid))
    Wa, Wb, bb = _normal(rng, (ms, L), L ** -0.5), _normal(rng, (T, ms), ms ** -0.5), _normal(rng, (T,), 0.5)
    cot = torch.from_numpy(rng.standard_normal((B * N, mid)))
    idxs = [_sa_idx(rng, B, N, k)]
    if k == N and N > 1:                                                 # every point neighbours every point
        idxs.append(torch.stack([torch.stack([torch.from_numpy(rng.permutation(N)) for _ in range(N)]) for _ in range(B)]).int())
    if N == 1:
        idxs.append(torch.full((B, N, k), -1, dtype=torch.int32))        # nothing but an out-of-range index
    for idx in idxs:
        def fn(Pr, Pin, dec):
            return R.sa_core(Pin, idx, Pr["Wa"], Pr["Wb"], Pr["bb"], rel, mid, share, dec)
        Pr = {"Wa": Wa, "Wb": Wb, "bb": bb}
        r64, r32 = R.run(fn, Pr, [P]), R.run(fn, Pr, [P], dtype=torch.float32)
        g = [t.to(dev).requires_grad_(True) for t in (P, Wa, Wb, bb)]
        rec = {}
        o = V.SaFn.apply(g[0], idx.to(dev), g[1], g[2], g[3], rel, mid, share, rec)
        what = f"sa {B}x{N} k{k} rel{rel} mid{mid}"
        check(WORST, "sa_fwd", what, o, r32["out"], r64["out"], F_FWD)
        force = {"sa.P": r64["dec"].mask["sa.P"]}                        # decided by the input alone
        force["sa.h"] = _mask_check(what, rec["h"] > 0, r32["dec"], r64["dec"], "sa.h")
        force["sa.o"] = _mask_check(what, rec["o"] > 0, r32["dec"], r64["dec"], "sa.o")
        f64, f32 = R.run(fn, Pr, [P], cot, force=force), R.run(fn, Pr, [P], cot, torch.float32, force)
        grads = torch.autograd.grad((o * cot.float().to(dev)).sum(), g)
        for name, got in zip(("in0", "Wa", "Wb", "bb"), grads):
            check(WORST, "sa_bwd", f"{what} d{name}", got, f32["grads"][name], f64["grads"][name], F_GRAD)
        named = torch.zeros(B, N, dtype=torch.bool)
        ok = (idx >= 0) & (idx < N)
        for b in range(B):
            named[b, idx[b][ok[b]].long()] = True
        lone = ~named.view(-1)
        if bool(lone.any()):                                             # a point no row names: exact zeros
            assert bool((grads[0][lone.to(dev), rel:] == 0).all())
        again = torch.autograd.grad((V.SaFn.apply(g[0], idx.to(dev), g[1], g[2], g[3], rel, mid, share) *
                                     cot.float().to(dev)).sum(), g)
        assert all(torch.equal(a, b) for a, b in zip(grads, again))


# ---------------- EdgePoolFn ----------------

@pytest.mark.parametrize("B,N,S,pk,C", [(1, 1, 1, 1, 1), (2, 17, 7, 4, 130), (1, 64, 32, 32, 64)])
def test_edge_pool(V, dev, B, N, S, pk, C):
    rng = np.random.default_rng(N * 10 + pk)
    feat = _eighths(rng, (B, N, C), -2, 3)                               # few values: many ties
    p_idx = torch.from_numpy(rng.integers(0, N, size=(B, S))).int()
    if S > 1:
        p_idx[:, 1] = p_idx[:, 0]                                        # a duplicate centre
    pn_idx = torch.from_numpy(rng.integers(0, N, size=(B, S, pk))).int()
    if pk > 1:
        pn_idx[:, :, pk - 1] = pn_idx[:, :, 0]                           # a tie by construction
    cot = _eighths(rng, (B * S, 2 * C))

    def fn(Pr, f, dec):
        return R.edge_pool(f, p_idx, pn_idx, dec)[0]
    r64 = R.run(fn, {}, [feat], cot)
    fd = feat.float().to(dev).requires_grad_(True)
    out, slot = V.EdgePoolFn.apply(fd, p_idx.to(dev), pn_idx.to(dev))
    assert slot.dtype == torch.uint8 and tuple(slot.shape) == (B, S, C)
    assert torch.equal(out.detach().cpu().double(), r64["out"])          # eighths: exact in both precisions
    assert torch.equal(slot.cpu().long(), r64["dec"].idx["slot"]), "the lowest j must win a tie"
    grad, = torch.autograd.grad((out * cot.float().to(dev)).sum(), fd)
    assert torch.equal(grad.cpu().double(), r64["grads"]["in0"])
    again, = torch.autograd.grad((V.EdgePoolFn.apply(fd, p_idx.to(dev), pn_idx.to(dev))[0] * cot.float().to(dev)).sum(), fd)
    assert torch.equal(grad, again)


# ---------------- UnpoolFn ----------------

@pytest.mark.parametrize("S", [1, 2, 3, 40])
@pytest.mark.parametrize("D1", [0, 5])
def test_unpool(V, dev, S, D1):
    """K = min(3, S) columns: fewer than three coarse points give fewer terms, never a padded neighbour."""
    from chamfer3D.model_utils import three_nn_upsampling
    rng = np.random.default_rng(S * 10 + D1)
    B, N, D2 = 2, 67, 6
    src, tgt = _normal(rng, (B, S, 3)), _normal(rng, (B, N, 3))
    tgt[:, 0] = src[:, 0]                                                # a fine point on a coarse one: the 1e-10 clamp
    feat2, skip = _normal(rng, (B, S, D2)), (_normal(rng, (B, N, D1)) if D1 else None)
    cot = torch.from_numpy(rng.standard_normal((B * N, D2 + D1)))
    K_ = min(3, S)
    idx, w = three_nn_upsampling(tgt.to(dev), src.to(dev))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, N, K_) == tuple(w.shape)
    want_idx, _ = R.knn_pick(tgt.double(), src.double(), K_)
    assert torch.equal(idx.cpu().long(), want_idx)
    w64, w32 = R.three_nn_weights(tgt.double(), src.double(), want_idx), R.three_nn_weights(tgt, src, want_idx)
    check(WORST, "unpool", f"weights S{S}", w, w32, w64, F_FWD)
    wg = w.detach().cpu()                                                # the interpolation itself under the given weights

    def fn(Pr, f2, *rest):
        sk, dec = (rest[0], rest[1]) if D1 else (None, rest[0])
        return R.unpool(f2, want_idx, wg.to(f2.dtype), sk)
    ins = [feat2] + ([skip] if D1 else [])
    r64, r32 = R.run(fn, {}, ins, cot), R.run(fn, {}, ins, cot, torch.float32)
    g = [t.to(dev).requires_grad_(True) for t in ins]
    out = V.UnpoolFn.apply(g[0], idx, w, g[1] if D1 else None)
    check(WORST, "unpool", f"fwd S{S} D1{D1}", out, r32["out"], r64["out"], F_FWD)
    if D1:                                                               # the column order of torch.cat([interp, skip], 1)
        interp = V.UnpoolFn.apply(g[0], idx, w, None)
        assert torch.equal(out.detach(), torch.cat((interp.detach(), g[1].detach().view(B * N, D1)), 1))
    grads = torch.autograd.grad((out * cot.float().to(dev)).sum(), g)
    for i, got in enumerate(grads):
        check(WORST, "unpool", f"bwd S{S} D1{D1} in{i}", got, r32["grads"][f"in{i}"], r64["grads"][f"in{i}"], F_GRAD)
    again = torch.autograd.grad((V.UnpoolFn.apply(g[0], idx, w, g[1] if D1 else None) * cot.float().to(dev)).sum(), g)
    assert all(torch.equal(a, b) for a, b in zip(grads, again))


# ---------------- SK selection passes ----------------

@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("C", [3, 130])
def test_sk_passes(V, dev, m, N, C):
    rng = np.random.default_rng(m * 1000 + N * 10 + C)
    B = 2
    ys = [_normal(rng, (B * N, C)) for _ in range(m)]
    a = torch.softmax(_normal(rng, (B, m, C)), 1)
    cs, cv = torch.from_numpy(rng.standard_normal((B, C))), torch.from_numpy(rng.standard_normal((B * N, C)))
    gy = [y.to(dev).requires_grad_(True) for y in ys]
    ga = a.to(dev).requires_grad_(True)

    def mean_fn(Pr, *rest):
        return R.sk_mean(rest[:-1], B)
    r64, r32 = R.run(mean_fn, {}, ys, cs), R.run(mean_fn, {}, ys, cs, torch.float32)
    s = V.SkMeanFn.apply(B, *gy)
    check(WORST, "sk", f"mean m{m} N{N} C{C}", s, r32["out"], r64["out"], F_FWD)
    grads = torch.autograd.grad((s * cs.float().to(dev)).sum(), gy)
    for i, got in enumerate(grads):
        check(WORST, "sk", f"mean bwd m{m} N{N} C{C} y{i}", got, r32["grads"][f"in{i}"], r64["grads"][f"in{i}"], F_GRAD)
    for relu_out in (False, True):
        def mix_fn(Pr, aa, *rest):
            return R.sk_mix(aa, rest[:-1], B, relu_out)
        r64, r32 = R.run(mix_fn, {}, [a] + ys, cv), R.run(mix_fn, {}, [a] + ys, cv, torch.float32)
        v = V.SkMixFn.apply(ga, relu_out, *gy)
        what = f"mix m{m} N{N} C{C} relu{int(relu_out)}"
        check(WORST, "sk", what, v, r32["out"], r64["out"], F_FWD)
        if relu_out:                                   # the trailing ReLU's mask under the tolerance rule ...
            pre64, pre32 = R.sk_mix(a.double(), [y.double() for y in ys], B), R.sk_mix(a, ys, B)
            gm = v.detach().cpu() > 0
            diff = gm != (pre64 > 0)
            assert not bool((diff & (pre64.abs() >= _tol(pre32, pre64))).any())
            assert int(diff.sum()) <= MASK_CAP * diff.numel()

            def mix_forced(Pr, aa, *rest):             # ... and the float64 backward under the GPU's mask
                return R.sk_mix(aa, rest[:-1], B, True, gm)
            r64, r32 = R.run(mix_forced, {}, [a] + ys, cv), R.run(mix_forced, {}, [a] + ys, cv, torch.float32)
        grads = torch.autograd.grad((v * cv.float().to(dev)).sum(), [ga] + gy)
        for i, got in enumerate(grads):
            check(WORST, "sk", f"{what} bwd in{i}", got, r32["grads"][f"in{i}"], r64["grads"][f"in{i}"], F_GRAD)
        again = torch.autograd.grad((V.SkMixFn.apply(ga, relu_out, *gy) * cv.float().to(dev)).sum(), [ga] + gy)
        assert all(torch.equal(p, q) for p, q in zip(grads, again))
    if m == 1:                                         # one branch: the attention is exactly 1
        one = torch.softmax(torch.stack([_normal(rng, (B, C)).to(dev)], 1), 1)
        assert bool((one == 1).all())
        assert torch.equal(V.SkMixFn.apply(one, False, gy[0]).detach(), torch.relu(gy[0].detach()))


# ---------------- helpers of chamfer3D/model_utils.py ----------------

def test_get_edge_features(V, dev):
    from chamfer3D.model_utils import get_edge_features
    rng = np.random.default_rng(5)
    B, C, N, k = 2, 7, 19, 4
    x = _normal(rng, (B, C, 1, N))
    idx = torch.from_numpy(rng.integers(0, N, size=(B, N, k)))
    got = get_edge_features(x.to(dev), idx.to(dev))
    want = R.gather_rows(x.squeeze(2).transpose(1, 2), idx).permute(0, 3, 2, 1)          # [B, C, k, N]
    assert tuple(got.shape) == (B, C, k, N) and torch.equal(got.cpu(), want)


def test_knn_in_six_dimensions(V, dev):
    """D != 3 goes through vn.knn_rows; (direct squared distance, index) order, the query itself first."""
    from chamfer3D.model_utils import knn
    B, D, N, k = 2, 6, 40, 5
    x = R.make_features(11, B, D, N)
    want, gap = R.knn_pick(x.transpose(1, 2).double(), x.transpose(1, 2).double(), k)
    assert gap >= R.GEO_MARGIN, "the inputs must keep every rank apart"
    got = knn(x.to(dev), k)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert torch.equal(got[:, :, 0].cpu(), torch.arange(N).expand(B, N))


def test_edge_preserve_sampling(V, dev):
    """The helper's four returns at the encoder fixture's first pooling (64 -> 32 points, pk 4), whose
    geometric decisions keep a margin of GEO_MARGIN."""
    from chamfer3D.model_utils import edge_preserve_sampling
    E = R.ENC
    B, N, S, pk, C = E["B"], E["pts_num"][0], E["pts_num"][1], E["pk"], 9
    pts = R.make_points(R.GOLDEN_SEED, B, N)
    rng = np.random.default_rng(6)
    feat = _eighths(rng, (B, C, N))
    cot = _eighths(rng, (B, 2 * C, S))
    p_want, g1 = R.fps_pick(pts.double(), S)
    out_want = torch.gather(pts, 1, p_want.unsqueeze(-1).expand(-1, -1, 3))
    pn_want, g2 = R.knn_pick(out_want.double(), pts.double(), pk)
    assert min(g1, g2) >= R.GEO_MARGIN
    fd = feat.float().to(dev).requires_grad_(True)
    net, p_idx, pn_idx, out_pts = edge_preserve_sampling(fd, pts.to(dev), S, pk)
    assert p_idx.dtype == torch.int32 and torch.equal(p_idx.cpu().long(), p_want)
    assert pn_idx.dtype == torch.int32 and torch.equal(pn_idx.cpu().long(), pn_want)
    assert torch.equal(out_pts.cpu(), out_want)

    def fn(Pr, f, dec):
        return R.edge_pool(f.transpose(1, 2), p_want, pn_want, dec)[0].view(B, S, 2 * C).transpose(1, 2)
    r64 = R.run(fn, {}, [feat], cot)
    assert tuple(net.shape) == (B, 2 * C, S) and torch.equal(net.detach().cpu().double(), r64["out"])
    grad, = torch.autograd.grad((net * cot.float().to(dev)).sum(), fd)
    assert torch.equal(grad.cpu().double(), r64["grads"]["in0"])


# ---------------- modules ----------------

def _build(name, dev):
    from models import vrcnet as M
    S, U, E = R.SA, R.UNIT, R.ENC
    if name == "sa":
        mod = M.SA_module(S["in_planes"], S["rel"], S["mid"], S["out_planes"], S["share"], S["k"])
    elif name == "sk":
        mod = M.SK_SA_module(S["in_planes"], S["rel"], S["mid"], S["out_planes"], S["share"], R.SK["k"])
    elif name == "unit":
        mod = M.SKN_Res_unit(U["input_size"], U["output_size"], U["k"], U["layers"])
    else:
        mod = M.SA_SKN_Res_encoder(E["C_in"], E["k"], E["pk"], E["output_size"], E["layers"], E["pts_num"])
    mod.load_state_dict(R.fixture(name)[0], strict=True)                 # reference keys, strict
    return mod.to(dev).eval()


@pytest.fixture(scope="module")
def refs():
    return {(n, d): R.run_fixture(n, d) for n in ("sa", "sk", "unit", "enc") for d in (torch.float64, torch.float32)}


def _forced(what, pre_gpu, d32, d64):
    """The GPU's ReLU masks, each checked against float64's -> the force dict of the float64 backward."""
    force = {}
    for name in d64.mask:
        t = pre_gpu[name].detach()
        ref = d64.pre[name]
        if t.dim() == 2 and ref.dim() == 2 and t.shape[1] != ref.shape[1]:
            t = t[:, :ref.shape[1]]                                      # '.P': only x1 | x2p pass a ReLU
        force[name] = _mask_check(what, t > 0, d32, d64, name)
    return force


def _grads_check(what, mod, xg, out, name, force, fam):
    Pr, _, _, cot = R.fixture(name)
    f64, f32 = R.run_fixture(name, force=force), R.run_fixture(name, torch.float32, force)
    params = dict(mod.named_parameters())
    got = torch.autograd.grad((out * cot.float().to(out.device)).sum(), [xg] + list(params.values()))
    check(WORST, fam, f"{what} dx", got[0], f32["grads"]["in0"], f64["grads"]["in0"], F_GRAD)
    for k, g in zip(params, got[1:]):
        check(WORST, fam, f"{what} d{k}", g, f32["grads"][k], f64["grads"][k], F_GRAD)


@pytest.mark.parametrize("name", ["sa", "sk", "unit"])
def test_units_against_the_restatement(V, dev, refs, name):
    r64, r32 = refs[name, torch.float64], refs[name, torch.float32]
    Pr, x, idxs, cot = R.fixture(name)
    B, N = x.shape[0], x.shape[3]
    mod = _build(name, dev)
    assert all(torch.equal(v.cpu(), Pr[k]) for k, v in mod.state_dict().items())
    mod.decisions = {}
    xg = x.to(dev).requires_grad_(True)
    di = [i.to(dev) for i in idxs]
    if name == "sa":
        out = mod([xg, di[0]])[0]
        rows = mod.forward_rows(R.to_rows(xg), di[0].int())
    elif name == "sk":
        out = mod([xg, di])[0]
        rows = mod.forward_rows(R.to_rows(xg), [i.int() for i in di], B)
    else:
        out = mod(xg, di)
        rows = mod.forward_rows(R.to_rows(xg), [i.int() for i in di], B)
    assert tuple(out.shape) == tuple(r64["out"].shape)
    check(WORST, "unit_fwd", f"{name} forward", out, r32["out"], r64["out"], F_FWD)
    assert torch.equal(R.from_rows(rows, B).detach(), out.detach()), "forward and forward_rows must agree bit for bit"
    force = _forced(name, mod.decisions["pre"], r32["dec"], r64["dec"])
    _grads_check(name, mod, xg, out, name, force, "unit_bwd")


def test_encoder_against_the_restatement(V, dev, refs):
    r64, r32 = refs["enc", torch.float64], refs["enc", torch.float32]
    d64, d32 = r64["dec"], r32["dec"]
    Pr, x, _, cot = R.fixture("enc")
    E = R.ENC
    B = E["B"]
    mod = _build("enc", dev)
    mod.decisions = {}
    xg = x.to(dev).requires_grad_(True)
    out = mod(xg)
    assert tuple(out.shape) == (B, E["output_size"], E["pts_num"][0])
    check(WORST, "enc_fwd", "encoder forward", out, r32["out"], r64["out"], F_FWD)
    rec = mod.decisions
    for lv in range(4):                                                  # the geometry: exact
        for i in range(len(E["k"])):
            assert torch.equal(rec["knn"][lv][i].cpu().long(), d64.idx[f"knn{lv + 1}.{i}"]), (lv, i)
    for lv in (1, 2, 3):
        assert torch.equal(rec["fps"][lv - 1].cpu().long(), d64.idx[f"fps{lv}"]), lv
        assert torch.equal(rec["pn_idx"][lv - 1].cpu().long(), d64.idx[f"pn_idx{lv}"]), lv
    for i, lv in enumerate((2, 1, 0)):
        assert torch.equal(rec["three_nn"][i].cpu().long(), d64.idx[f"three_nn{lv}"]), lv
    force = _forced("enc", rec["pre"], d32, d64)
    for lv in (1, 2, 3):                                                 # pool slots: within twice the tolerance of the pooled layer
        got = rec["slot"][lv - 1].cpu().long()
        diff = got != d64.idx[f"slot{lv}"]
        tol = 2 * _tol(d32.pre[f"x{lv}"], d64.pre[f"x{lv}"])
        assert not bool((diff & (d64.margin[f"slot{lv}"] >= tol)).any()), lv
        assert int(diff.sum()) <= MASK_CAP * diff.numel(), lv
        force[f"slot{lv}"] = got
    n4 = E["pts_num"][3]
    win = rec["win"].cpu().long() - torch.arange(B).view(B, 1) * n4
    assert bool(((win >= 0) & (win < n4)).all())
    diff = win != d64.idx["win"]
    tol = 2 * _tol(d32.pre["conv5"], d64.pre["conv5"])
    assert not bool((diff & (d64.margin["win"] >= tol)).any()), "a conv5 winner differs beyond twice the forward tolerance"
    assert int(diff.sum()) <= MASK_CAP * diff.numel()
    force["win"] = win
    _grads_check("encoder", mod, xg, out, "enc", force, "enc_bwd")
    rows = mod.forward_rows(xg)
    assert torch.equal(R.from_rows(rows, B, four=False).detach(), out.detach())


def test_encoder_train_mode_differs_only_through_dropout(V, dev):
    mod = _build("enc", dev)
    x = R.fixture("enc")[1].to(dev)
    with torch.no_grad():
        ev = mod(x)
        mod.train()
        mod.dropout.p = 0.0
        assert torch.equal(mod(x), ev), "with dropout disabled, train mode is eval mode"
        mod.dropout.p = 0.5
        torch.manual_seed(0)
        tr = mod(x)
        assert not torch.equal(tr, ev) and bool(torch.isfinite(tr).all())


def test_state_dict_round_trip(V, dev):
    mod = _build("enc", dev)
    sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    assert list(sd) == list(R.fixture("enc")[0])
    other = _build("enc", dev)
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(mod.state_dict().values(), other.state_dict().values()))


def test_sa_module_forward_memory(V, dev):
    """One SA_module forward at B 2, N 256, C 64, k 16 allocates less than one [B, C, k, N] float tensor."""
    from models import vrcnet as M
    B, N, C, k = 2, 256, 64, 16
    torch.manual_seed(1)
    mod = M.SA_module(C, C // 16, C // 4, C, 8, k).to(dev)
    x = torch.randn(B * N, C, device=dev, requires_grad=True)
    idx = torch.randint(0, N, (B, N, k), device=dev, dtype=torch.int32)
    mod.forward_rows(x, idx)                                             # warm the allocator's pools and the library
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = mod.forward_rows(x, idx)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    print(f"SA_module forward: {delta} bytes of new memory; one [B, C, k, N] float tensor is {B * C * k * N * 4}")
    assert y.shape == (B * N, C)
    assert delta < B * C * k * N * 4
