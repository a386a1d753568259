"""The PCN completion network on the GPU (csrc/pcn.hip, ured_hip/pcn.py, models/pcn.py) against
tests/pcn_ref.py in float64, which tests/test_pcn_ref.py pins to the reference's own modules.

Tolerance, from tests/tol_check.py: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|, f = 1e-5
forward and 2e-5 gradients; ref32 is the same restatement in float32 on the CPU. Nothing is derived
from the GPU's output. Decisions and backward as in tests/test_chain_gpu.py: the Functions record
their pre-activations and pool winners; a GPU ReLU mask or winner may differ from float64's own only
where the deciding value lies within the layer's forward tolerance of zero (twice that, of the
maximum, for a winner) and in at most MASK_CAP (0.05 %) of a layer's elements; the float64 backward
runs with the GPU's decisions forced under fixed random cotangents, and every input and parameter
gradient is compared as a whole tensor. The kernel-level inputs are small multiples of 1/8, so
every sum is exact in fp32 and in float64 alike.
"""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

import pcn_ref as R
from chain_ref import MASK_CAP
from tol_check import F_FWD, F_GRAD, FLOOR_MULT, check

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def Pn(dev):
    from ured_hip import pcn
    yield pcn
    for fam, (ratio, what) in sorted(WORST.items()):
        print(f"worst ratio {fam:14s} {ratio:.3f}  ({what})")


@pytest.fixture(autouse=True)
def _pcn_debug_word():
    """The debug build's bounds word of pcn.hip (file id 17), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_pcn"):
        return
    fn = mod._lib.ured_dbg_pcn
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): pcn.hip:{v & 0xFFFFFFFF}"


def _eighths(rng, shape, lo=-16, hi=17):
    return torch.from_numpy(rng.integers(lo, hi, size=shape).astype(np.float64) / 8)


# ---------------- kernels ----------------

@pytest.mark.parametrize("scale,B,nc,C", [(1, 1, 5, 512), (2, 3, 17, 512), (4, 2, 16, 130), (8, 2, 33, 512)])
def test_fold_and_center_kernels(Pn, dev, scale, B, nc, C):
    rng = np.random.default_rng(scale * 100 + nc)
    R_ = B * nc * scale
    Gb, Pc, Gs = _eighths(rng, (B, C)), _eighths(rng, (B * nc, C)), _eighths(rng, (scale, C))
    dH = _eighths(rng, (R_, C))
    f = lambda t: t.float().to(dev)                                                  # noqa: E731
    Y64 = ((Gb.view(B, 1, 1, C) + Pc.view(B, nc, 1, C)) + Gs.view(1, 1, scale, C)).reshape(R_, C)
    Y = Pn.fold_fwd(f(Gb), f(Pc), f(Gs), B, nc, scale)
    check(WORST, "pcn_fold", "fold_fwd", Y, Y64.float(), Y64, F_FWD)
    G = (dH * (Y64 > 0)).view(B, nc, scale, C)
    dGb, dPc, dGs = Pn.fold_bwd(f(dH), Y, B, nc, scale)
    for name, got, want in (("dGb", dGb, G.sum((1, 2))), ("dPc", dPc, G.sum(2).reshape(B * nc, C)),
                            ("dGs", dGs, G.sum((0, 1)))):
        check(WORST, "pcn_fold", f"fold_bwd {name}", got, want.float(), want, F_GRAD)
    again = Pn.fold_bwd(f(dH), Y, B, nc, scale)
    assert all(torch.equal(a, b) for a, b in zip((dGb, dPc, dGs), again))
    y3, cp, dF, add = _eighths(rng, (R_, 3)), _eighths(rng, (B * nc, 3)), _eighths(rng, (R_, 3)), _eighths(rng, (B * nc, 3))
    want = y3 + cp.repeat_interleave(scale, 0)
    check(WORST, "pcn_center", "center_fwd", Pn.center_fwd(f(y3), f(cp), B, nc, scale), want.float(), want, F_FWD)
    want = dF.view(B * nc, scale, 3).sum(1)
    check(WORST, "pcn_center", "center_bwd", Pn.center_bwd(f(dF), None, B, nc, scale), want.float(), want, F_GRAD)
    check(WORST, "pcn_center", "center_bwd + add", Pn.center_bwd(f(dF), f(add), B, nc, scale), (want + add).float(),
          want + add, F_GRAD)


@pytest.mark.parametrize("G,rows,C,n", [(1, 1, 3, 1), (3, 7, 130, 5), (2, 256, 64, 1027)])
def test_relu_and_pool_backward_kernels(Pn, dev, G, rows, C, n):
    rng = np.random.default_rng(G * 10 + rows)
    y, g = _eighths(rng, (n,)), _eighths(rng, (n,))
    yd, gd = y.float().to(dev), g.float().to(dev)
    assert torch.equal(Pn.relu(yd).cpu().double(), y.clamp(min=0))
    assert torch.equal(Pn.relu(yd, gd).cpu().double(), g * (y > 0))
    gp = _eighths(rng, (G, C))
    win = torch.from_numpy(rng.integers(0, rows, size=(G, C))) + torch.arange(G).view(G, 1) * rows
    want = torch.zeros(G * rows, C, dtype=torch.float64)
    for grp in range(G):
        want[win[grp], torch.arange(C)] = gp[grp]
    wd = win.to(torch.int32).to(dev)
    got = Pn.pool_bwd(gp.float().to(dev), wd, rows)
    assert torch.equal(got.cpu().double(), want)
    base = _eighths(rng, (G * rows, C))
    got = Pn.pool_bwd(gp.float().to(dev), wd, rows, base.float().to(dev))
    assert torch.equal(got.cpu().double(), base + want)


# ---------------- decisions ----------------

def _pm(t):
    """[B,C,N] -> point-major [B*N, C]."""
    return t.transpose(1, 2).reshape(-1, t.shape[1])


def _tol(a32, a64, f):
    return FLOOR_MULT * (a32.double() - a64).abs().max().item() + f * a64.abs().max().item()


def _check_relu_layer(what, key, Ygpu, r32, r64, to_ref):
    """Forward value, then the GPU's mask against float64's. -> the mask in the reference's layout."""
    p32, p64 = r32["pre"][key], r64["pre"][key]
    pm = (lambda t: t) if p64.dim() == 2 else _pm
    check(WORST, "pcn_fwd", f"{what} {key}", Ygpu, pm(p32), pm(p64), F_FWD)
    m = (Ygpu > 0).cpu()
    diff = m != pm(p64 > 0)
    n = int(diff.sum())
    print(f"{what} {key}: {n} of {m.numel()} masks differ from float64")
    assert n <= MASK_CAP * m.numel(), f"{what} {key}: {n} of {m.numel()} ReLU masks differ"
    if n:
        worst, tol = pm(p64)[diff].abs().max().item(), _tol(p32, p64, F_FWD)
        assert worst <= tol, f"{what} {key}: a mask differs where |z| = {worst:.3e} > {tol:.3e}"
    return to_ref(m)


def _check_winners(what, ykey, wkey, Ygpu, win_gpu, r32, r64, N):
    p32, p64 = r32["pre"][ykey], r64["pre"][ykey]
    check(WORST, "pcn_fwd", f"{what} {ykey}", Ygpu, _pm(p32), _pm(p64), F_FWD)
    B, C = win_gpu.shape
    w = (win_gpu.cpu().long() - torch.arange(B).view(B, 1) * N)
    assert bool(((w >= 0) & (w < N)).all()), f"{what} {wkey}: a winner outside its cloud"
    chosen = p64.gather(2, w.unsqueeze(2)).squeeze(2)
    gap = (p64.amax(2) - chosen).max().item()
    tol = _tol(p32, p64, F_FWD)
    n = int((w != r64["pre"][wkey]).sum())
    print(f"{what} {wkey}: {n} of {w.numel()} winners differ, largest gap {gap:.3e} (allowed {2 * tol:.3e})")
    assert n <= MASK_CAP * w.numel() and gap <= 2 * tol
    return w


def _encoder_decisions(what, rec, r32, r64, B, N):
    un = lambda m: m.view(B, N, -1).transpose(1, 2)                                  # noqa: E731
    return {"Y1": _check_relu_layer(what, "Y1", rec["Y1"], r32, r64, un),
            "win1": _check_winners(what, "Y2", "win1", rec["Y2"], rec["win1"], r32, r64, N),
            "Y3": _check_relu_layer(what, "Y3", rec["Y3"], r32, r64, un),
            "win2": _check_winners(what, "Y4", "win2", rec["Y4"], rec["win2"], r32, r64, N)}


def _decoder_decisions(what, rec, r32, r64, B, nf):
    un = lambda m: m.view(B, nf, -1).transpose(1, 2)                                 # noqa: E731
    same = lambda m: m                                                               # noqa: E731
    return {"A1": _check_relu_layer(what, "A1", rec["A1"], r32, r64, same),
            "A2": _check_relu_layer(what, "A2", rec["A2"], r32, r64, same),
            "D1": _check_relu_layer(what, "D1", rec["Y1"], r32, r64, un),
            "D2": _check_relu_layer(what, "D2", rec["Y2"], r32, r64, un)}


def _load(mod, P, prefix, dev):
    mod.load_state_dict({k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}, strict=True)
    return mod.to(dev)


def _check_grads(what, named, r32, r64):
    for k, g in named.items():
        assert g is not None, f"{what}: no gradient for {k}"
        check(WORST, "pcn_bwd", f"{what} d{k}", g, r32["grads"][k], r64["grads"][k], F_GRAD)


# ---------------- encoder ----------------

@pytest.mark.parametrize("B,N", [(1, 1), (2, 48), (3, 130), (2, 256)])
def test_encoder(Pn, dev, B, N):
    from models.pcn import PCN_encoder
    seed = 10 + N
    P, x = R.make_params(seed, 16), R.make_input(seed, B, N)
    cot = torch.from_numpy(np.random.default_rng(seed).standard_normal((B, 1024)))
    enc = _load(PCN_encoder(), P, "encoder.", dev)
    xg = x.to(dev).requires_grad_(True)
    what = f"encoder {B}x{N}"

    def once():
        rec = {}
        enc.zero_grad(set_to_none=True)
        xg.grad = None
        feat = enc(xg, rec)
        (feat * cot.float().to(dev)).sum().backward()
        return feat, rec, {**{"encoder." + k: p.grad for k, p in enc.named_parameters()}, "x": xg.grad}

    feat, rec, grads = once()
    r64, r32 = R.run_encoder(P, x), R.run_encoder(P, x, dtype=torch.float32)
    check(WORST, "pcn_fwd", f"{what} feature", feat, r32["feat"], r64["feat"], F_FWD)
    dec = _encoder_decisions(what, rec, r32, r64, B, N)
    _check_grads(what, grads, R.run_encoder(P, x, cot, torch.float32, dec), R.run_encoder(P, x, cot, dec=dec))
    feat2, _, grads2 = once()
    assert torch.equal(feat, feat2) and all(torch.equal(grads[k], grads2[k]) for k in grads), f"{what}: two runs differ"


# ---------------- decoder and the whole network ----------------

@pytest.mark.parametrize("B,N,nc,scale", [(2, 48, 16, 4), (3, 48, 33, 2)])
def test_decoder_and_network(Pn, dev, B, N, nc, scale):
    from models.pcn import PCN_decoder, PCN_encoder
    seed = R.GOLDEN_SEED if nc == 16 else 5
    nf = nc * scale
    P, x = R.make_params(seed, nc), R.make_input(seed, B, N)
    cot = R.cotangents(seed, B, nc, nf)
    enc = _load(PCN_encoder(), P, "encoder.", dev)
    decm = _load(PCN_decoder(nc, nf, scale, 1029), P, "decoder.", dev)
    assert torch.equal(decm.grid.cpu(), R.gen_grid_up(scale, 0.05))
    r64, r32 = R.run(P, x, nc, scale), R.run(P, x, nc, scale, dtype=torch.float32)
    cc, cf = cot[0].float().to(dev), cot[1].float().to(dev)

    # the decoder alone, on float64's feature
    what = f"decoder {B}x{nc}x{scale}"
    fg = r64["feat"].float().to(dev).requires_grad_(True)
    rec = {}
    coarse, fine = decm(fg, rec)
    assert coarse.shape == (B, 3, nc) and fine.shape == (B, 3, nf)
    ((coarse * cc).sum() + (fine * cf).sum()).backward()
    d64, d32 = R.run(P, None, nc, scale, feat_in=r64["feat"]), R.run(P, None, nc, scale, dtype=torch.float32, feat_in=r64["feat"])
    check(WORST, "pcn_fwd", f"{what} coarse", coarse, d32["coarse"], d64["coarse"], F_FWD)
    check(WORST, "pcn_fwd", f"{what} fine", fine, d32["fine"], d64["fine"], F_FWD)
    dec = _decoder_decisions(what, rec, d32, d64, B, nf)
    g = {**{"decoder." + k: p.grad for k, p in decm.named_parameters()}, "feat": fg.grad}
    _check_grads(what, g, R.run(P, None, nc, scale, cot, torch.float32, dec, feat_in=r64["feat"]),
                 R.run(P, None, nc, scale, cot, dec=dec, feat_in=r64["feat"]))

    # the whole network
    what = f"network {B}x{N}x{nc}x{scale}"
    xg = x.to(dev).requires_grad_(True)

    def once():
        rec_e, rec_d = {}, {}
        enc.zero_grad(set_to_none=True)
        decm.zero_grad(set_to_none=True)
        xg.grad = None
        coarse, fine = decm(enc(xg, rec_e), rec_d)
        ((coarse * cc).sum() + (fine * cf).sum()).backward()
        g = {"encoder." + k: p.grad for k, p in enc.named_parameters()}
        g.update({"decoder." + k: p.grad for k, p in decm.named_parameters()})
        g["x"] = xg.grad
        return coarse, fine, rec_e, rec_d, g

    coarse, fine, rec_e, rec_d, g = once()
    check(WORST, "pcn_fwd", f"{what} coarse", coarse, r32["coarse"], r64["coarse"], F_FWD)
    check(WORST, "pcn_fwd", f"{what} fine", fine, r32["fine"], r64["fine"], F_FWD)
    dec = {**_encoder_decisions(what, rec_e, r32, r64, B, N), **_decoder_decisions(what, rec_d, r32, r64, B, nf)}
    _check_grads(what, g, R.run(P, x, nc, scale, cot, torch.float32, dec), R.run(P, x, nc, scale, cot, dec=dec))
    again = once()
    assert torch.equal(fine, again[1]) and all(torch.equal(g[k], again[4][k]) for k in g), f"{what}: two runs differ"


# ---------------- Model wiring ----------------

def _args(loss, num_points=64, eval_emd=True):
    return types.SimpleNamespace(num_points=num_points, loss=loss, eval_emd=eval_emd, loss_opts={"alpha": 200, "lambda": 0.5})


def _pair(dev, B=2, n=64):
    """A cloud and its occluded view (ured_hip.occ.occlude keeps n // 2 points)."""
    from ured_hip import occ
    r = np.random.Generator(np.random.PCG64(77))
    gt = torch.from_numpy(r.random((B, n, 3), dtype=np.float32) - np.float32(0.5)).to(dev)
    z = torch.zeros(B, n, dtype=torch.int64, device=dev)
    part = occ.occlude(gt, z, z, seed=5)["ori_point_occ"]
    return part.transpose(1, 2).contiguous(), gt


@pytest.mark.parametrize("loss", ["cd", "dcd", "emd"])
def test_model_training_wiring(Pn, dev, loss):
    from chamfer3D.model_utils import calc_cd, calc_dcd, calc_emd
    from models.pcn import Model
    torch.manual_seed(0)
    m = Model(_args(loss), num_coarse=16).to(dev)
    x, gt = _pair(dev)
    alpha = 0.5

    def once():
        m.zero_grad(set_to_none=True)
        out2, loss2, total, none = m(x, gt, is_training=True, alpha=alpha)
        total.backward()
        return out2, loss2, total, none, [p.grad.clone() for p in m.parameters()]

    out2, loss2, total, none, grads = once()
    assert none is None and out2.shape == (2, 64, 3) and loss2.shape == (2,)
    with torch.no_grad():
        feat = m.encoder(x)
        out1 = m.decoder(feat)[0].transpose(1, 2).contiguous()
        o2 = out2.detach()
        if loss == "cd":
            l1, l2 = calc_cd(out1, gt)[0], calc_cd(o2, gt)[0]
        elif loss == "dcd":
            l1, l2 = calc_dcd(out1, gt, alpha=200, n_lambda=0.5)[0], calc_dcd(o2, gt, alpha=200, n_lambda=0.5)[0]
        else:
            l1, l2 = calc_cd(out1, gt)[0], calc_emd(o2, gt)[0]
    want, got = float(l1.mean() + alpha * l2.mean()), float(total.detach())
    assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), (got, want)
    assert torch.allclose(loss2.detach(), l2, rtol=0, atol=2e-6)
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    again = once()
    assert torch.equal(total, again[2]) and all(torch.equal(a, b) for a, b in zip(grads, again[4])), "two runs differ"
    with pytest.raises(ValueError, match="alpha"):
        m(x, gt, is_training=True)


def test_model_evaluation_and_state_dict(Pn, dev):
    from models.pcn import Model
    m = Model(_args("dcd"), num_coarse=16).to(dev)
    P = R.make_params(3, 16)
    m.load_state_dict(P, strict=True)
    sd = m.state_dict()
    assert list(sd) == R.ENC_KEYS + R.DEC_KEYS and all(torch.equal(sd[k].cpu(), P[k]) for k in P)
    x, gt = _pair(dev)
    with torch.no_grad():
        res = m(x, gt, is_training=False)
        res2 = m(x, gt, is_training=False, test_emd=False)
    assert list(res) == ["out1", "out2", "emd", "dcd", "cd_t", "f1"]
    assert res["out1"].shape == (2, 16, 3) and res["out2"].shape == (2, 64, 3)
    assert res["emd"].shape == (2,) and res["dcd"].shape == (2,) and res["cd_t"].shape == (2,) and res["f1"].shape == (2,)
    assert res2["emd"].shape == (1,) and float(res2["emd"]) == 1.0
    assert all(bool(torch.isfinite(v).all()) for v in res.values())


def test_five_adam_steps(Pn, dev):
    from models.pcn import Model
    torch.manual_seed(1)
    m = Model(_args("dcd"), num_coarse=16).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    x, gt = _pair(dev)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        _, _, total, _ = m(x, gt, is_training=True, alpha=0.5)
        total.backward()
        opt.step()
        losses.append(float(total.detach()))
    assert all(np.isfinite(losses)), losses
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
