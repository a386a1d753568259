"""VRCNet's Model on the GPU (the latent / Gaussian kernels of csrc/vrc.hip, LatentFn and GaussKernelFn in
ured_hip/vrc.py, Model in models/vrcnet.py) against tests/vrcmodel_ref.py in float64, which
tests/test_vrcmodel_ref.py pins to the reference's own Model.

Tolerance: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64| (tests/tol_check.py; F_FWD forward, F_GRAD
gradients), whole tensors. The FPS picks of y and the nearest-neighbour picks of the loss heads are compared
exactly (the fixture keeps them away from a flip, tests/vrcmodel_ref.py).

Raw scales of +-30 and -80 enter the forward (and the z-only backward) only where float32 can hold the result:
s = softplus(-30) = 9.4e-14 gives a KL gradient of the order 1 / s^3 = 1e39, beyond float32 in any
implementation, and softplus(-80) = 1.8e-35 squares to 0, so -80 is checked in the evaluation form and +-30 in
the forward and under dz alone.
"""
import ctypes
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

import vrc_ref as R
import vrcmodel_ref as M
from conftest import GOLDEN
from tol_check import F_FWD, F_GRAD, check

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
def gold():
    return dict(np.load(os.path.join(GOLDEN, "vrcmodel.npz")))


@pytest.fixture(scope="module")
def refs():
    """Computed once, shared, never modified."""
    return {(c, s, d): M.run_fixture(c, d, s) for c in M.COMBOS for s in (False, True) for d in (torch.float64, torch.float32)}


def _normal(rng, shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) * scale


# ---------------- the latent kernels ----------------

LATENT_SHAPES = [(1, 1), (3, 130), (2, 128), (5, 4096)]
THRESHOLD = [20.0, 20.0 + 1e-3, 20.0 - 1e-3]
EXTREME = [30.0, -30.0]


def _plant(o, Z, values, col=0):
    """Write `values` into the raw-scale half of o, one per element starting at (row 0, column col), wrapping."""
    flat = o[:, Z:].reshape(-1).clone()
    for i, v in enumerate(values):
        flat[(col + i) % flat.numel()] = v
    o[:, Z:] = flat.view(o.shape[0], Z)
    return o


def _latent_inputs(B, Z, values_q, values_p):
    rng = np.random.default_rng(B * 10000 + Z)
    oq, op = _normal(rng, (B, 2 * Z)), _normal(rng, (B, 2 * Z))
    _plant(oq, Z, values_q, 0)
    _plant(op, Z, values_p, 1)
    return oq, op, _normal(rng, (B, Z)), _normal(rng, (B, Z)), rng


def _latent_ref(oq, op, eq, ep, cots, dtype):
    """-> (outputs, grads) of the restatement under the cotangents (None = absent)."""
    a = oq.detach().clone().to(dtype).requires_grad_(True)
    b = None if op is None else op.detach().clone().to(dtype).requires_grad_(True)
    outs = M.latent(a, b, eq.to(dtype), None if ep is None else ep.to(dtype))
    total = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots) if c is not None)
    leaves = [a] + ([] if b is None else [b])
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
    return [None if o is None else o.detach() for o in outs], grads


def _latent_gpu(V, dev, oq, op, eq, ep, cots):
    a = oq.to(dev).requires_grad_(True)
    b = None if op is None else op.to(dev).requires_grad_(True)
    outs = V.LatentFn.apply(a, b, eq.to(dev), None if ep is None else ep.to(dev))
    total = sum((o * c.float().to(dev)).sum() for o, c in zip(outs, cots) if c is not None)
    total.backward()
    return outs, [a.grad] + ([] if b is None else [b.grad])


def _latent_case(V, dev, what, oq, op, eq, ep, cots, fwd=True):
    r64, g64 = _latent_ref(oq, op, eq, ep, cots, torch.float64)
    r32, g32 = _latent_ref(oq, op, eq, ep, cots, torch.float32)
    outs, grads = _latent_gpu(V, dev, oq, op, eq, ep, cots)
    if fwd:
        for name, o, a32, a64 in zip(("z", "kl_rec", "kl_g"), outs, r32, r64):
            assert (o is None) == (a64 is None)
            if o is not None:
                check(WORST, "latent_fwd", f"{what} {name}", o, a32, a64, F_FWD)
    for name, g, a32, a64 in zip(("d_oq", "d_op"), grads, g32, g64):
        check(WORST, "latent_bwd", f"{what} {name}", g, a32, a64, F_GRAD)
    return outs, grads


@pytest.mark.parametrize("B,Z", LATENT_SHAPES)
def test_latent_training(V, dev, B, Z):
    oq, op, eq, ep, rng = _latent_inputs(B, Z, THRESHOLD, THRESHOLD[::-1])
    cz, ckr, ckg = (torch.from_numpy(rng.standard_normal(s)) for s in ((2 * B, Z), (B, Z), (B, Z)))
    outs, grads = _latent_case(V, dev, f"train {B}x{Z}", oq, op, eq, ep, (cz, ckr, ckg))
    assert outs[0].shape == (2 * B, Z) and outs[1].shape == (B, Z) and outs[2].shape == (B, Z)
    again = _latent_gpu(V, dev, oq, op, eq, ep, (cz, ckr, ckg))
    assert all(torch.equal(a, b) for a, b in zip(outs, again[0])) and all(torch.equal(a, b) for a, b in zip(grads, again[1]))
    # every combination of absent cotangents (all absent: no backward runs at all)
    for present in itertools.product((True, False), repeat=3):
        if not any(present) or all(present):
            continue
        cots = tuple(c if p else None for c, p in zip((cz, ckr, ckg), present))
        _latent_case(V, dev, f"train {B}x{Z} cot {''.join('x' if p else '-' for p in present)}", oq, op, eq, ep, cots, fwd=False)
    # +-30: the forward, and the backward under dz alone (module docstring)
    oq, op, eq, ep, rng = _latent_inputs(B, Z, EXTREME, EXTREME[::-1])
    _latent_case(V, dev, f"train {B}x{Z} +-30", oq, op, eq, ep, (cz, None, None))


@pytest.mark.parametrize("B,Z", LATENT_SHAPES)
def test_latent_evaluation(V, dev, B, Z):
    oq, _, eq, _, rng = _latent_inputs(B, Z, THRESHOLD + EXTREME + [-80.0], [])
    cz = torch.from_numpy(rng.standard_normal((B, Z)))
    outs, grads = _latent_case(V, dev, f"eval {B}x{Z}", oq, None, eq, None, (cz, None, None))
    assert outs[0].shape == (B, Z) and outs[1] is None and outs[2] is None
    if Z > 5:                                          # the planted -80: the sigmoid is tiny (1.8e-35) but not zero
        assert 0 < float(grads[0][0, Z + 5].abs()) < 1e-30
    again = _latent_gpu(V, dev, oq, None, eq, None, (cz, None, None))
    assert torch.equal(outs[0], again[0][0]) and torch.equal(grads[0], again[1][0])


def test_latent_equal_distributions(V, dev):
    """mu_p == mu_q and s_p == s_q: kl_g stays within tolerance of 0 (it is exactly 0) and its gradient is finite."""
    oq, _, eq, ep, rng = _latent_inputs(3, 130, THRESHOLD, [])
    ck = torch.from_numpy(rng.standard_normal((3, 130)))
    outs, grads = _latent_case(V, dev, "equal", oq, oq.clone(), eq, ep, (None, None, ck))
    assert float(outs[2].detach().abs().max()) == 0.0
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[1].abs().max()) == 0.0     # the prior is detached in kl_g


def test_latent_limits(V, dev):
    from ured_hip import _lib
    z = torch.zeros
    with pytest.raises(ValueError, match="Z 4097 outside"):
        V.LatentFn.apply(z(1, 2 * 4097, device=dev), None, z(1, 4097, device=dev), None)
    with pytest.raises(ValueError, match="eps_q has shape"):
        V.LatentFn.apply(z(2, 8, device=dev), None, z(2, 3, device=dev), None)
    with pytest.raises(RuntimeError, match="MI355X only"):
        V.LatentFn.apply(z(2, 8, device=dev), None, z(2, 4), None)
    a = z(2, 8, device=dev)
    with pytest.raises(_lib.UredError, match="B 0 outside"):
        _lib.call("ured_vrc_latent_fwd", a.data_ptr(), None, a.data_ptr(), None, 0, 4, a.data_ptr(), None, None, None)
    with pytest.raises(_lib.UredError, match="needs eps_p"):
        _lib.call("ured_vrc_latent_fwd", a.data_ptr(), a.data_ptr(), a.data_ptr(), None, 2, 4, a.data_ptr(), None, None, None)
    with pytest.raises(_lib.UredError, match="no KL cotangents"):
        _lib.call("ured_vrc_latent_bwd", a.data_ptr(), None, a.data_ptr(), None, None, a.data_ptr(), None, 2, 4, a.data_ptr(),
                  None, None)


# ---------------- the Gaussian kernel ----------------

GAUSS_SHAPES = [(1, 1, 1), (3, 5, 7), (33, 33, 128), (64, 2, 130)]


def _gauss_ref(x, y, cot, dtype, same=False):
    a = x.detach().clone().to(dtype).requires_grad_(True)
    b = a if same else y.detach().clone().to(dtype).requires_grad_(True)
    K = M.gauss(a, b)
    g = torch.autograd.grad((K * cot.to(dtype)).sum(), [a] if same else [a, b])
    return K.detach(), list(g)


def _gauss_gpu(V, dev, x, y, cot, same=False):
    a = x.to(dev).requires_grad_(True)
    b = a if same else y.to(dev).requires_grad_(True)
    K = V.GaussKernelFn.apply(a, b)
    (K * cot.float().to(dev)).sum().backward()
    return K, [a.grad] if same else [a.grad, b.grad]


@pytest.mark.parametrize("n,m,Z", GAUSS_SHAPES)
def test_gauss(V, dev, n, m, Z):
    rng = np.random.default_rng(n * 1000 + m * 10 + Z)
    x, y = _normal(rng, (n, Z)), _normal(rng, (m, Z))
    y[0] = x[n - 1]                                    # one equal pair
    cot = torch.from_numpy(rng.standard_normal((n, m)))
    what = f"gauss {n}x{m}x{Z}"
    (K64, g64), (K32, g32) = _gauss_ref(x, y, cot, torch.float64), _gauss_ref(x, y, cot, torch.float32)
    K, g = _gauss_gpu(V, dev, x, y, cot)
    check(WORST, "gauss_fwd", f"{what} K", K, K32, K64, F_FWD)
    assert float(K[n - 1, 0]) == 1.0
    for name, a, a32, a64 in zip(("dx", "dy"), g, g32, g64):
        check(WORST, "gauss_bwd", f"{what} {name}", a, a32, a64, F_GRAD)
    K2, g2 = _gauss_gpu(V, dev, x, y, cot)
    assert torch.equal(K, K2) and all(torch.equal(a, b) for a, b in zip(g, g2)), "two runs differ"
    # x is y: a diagonal of exactly 1, and the gradient of both roles summed
    cot = torch.from_numpy(rng.standard_normal((n, n)))
    (K64, g64), (K32, g32) = _gauss_ref(x, x, cot, torch.float64, True), _gauss_ref(x, x, cot, torch.float32, True)
    K, g = _gauss_gpu(V, dev, x, x, cot, same=True)
    assert bool((K.diagonal() == 1.0).all())
    check(WORST, "gauss_fwd", f"{what} K(x, x)", K, K32, K64, F_FWD)
    check(WORST, "gauss_bwd", f"{what} dx of K(x, x)", g[0], g32[0], g64[0], F_GRAD)


def test_gauss_far_rows_and_eighths(V, dev):
    n, m, Z = 5, 4, 128
    x, y = torch.zeros(n, Z), torch.full((m, Z), 1e3)
    K, g = _gauss_gpu(V, dev, x, y, torch.ones(n, m, dtype=torch.float64))
    assert float(K.abs().max()) == 0.0
    assert all(bool(torch.isfinite(a).all()) and float(a.abs().max()) == 0.0 for a in g)
    # values on eighths, Z a power of two: every difference, square, the sum and both divisions are exact in
    # float32, so only expf's own error (1 ulp, HIP's documented bound) and the rounding of the float64 value
    # remain: 2 ulp of a result in (0, 1], 2^-23
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.integers(-16, 17, size=(n, Z)).astype(np.float32) / 8)
    y = torch.from_numpy(rng.integers(-16, 17, size=(m, Z)).astype(np.float32) / 8)
    K = V.GaussKernelFn.apply(x.to(dev), y.to(dev))
    err = (K.double().cpu() - M.gauss(x.double(), y.double())).abs().max().item()
    print(f"gauss eighths: err {err:.3e} bound {2.0 ** -23:.3e}")
    assert err <= 2.0 ** -23


def test_gauss_limits(V, dev):
    from ured_hip import _lib
    z = torch.zeros
    with pytest.raises(ValueError, match="outside"):
        V.GaussKernelFn.apply(z(1, 4097, device=dev), z(1, 4097, device=dev))
    with pytest.raises(ValueError, match="y has shape"):
        V.GaussKernelFn.apply(z(3, 4, device=dev), z(3, 5, device=dev))
    a = z(4, 4, device=dev)
    with pytest.raises(_lib.UredError, match="n 0 or m 4 outside"):
        _lib.call("ured_vrc_gauss_fwd", a.data_ptr(), a.data_ptr(), 0, 4, 4, a.data_ptr(), None)


@pytest.fixture(scope="module")
def net(dev, V):
    """One real Model at the golden's key shapes, for the methods that need an instance."""
    from models.vrcnet import Model
    torch.manual_seed(0)
    return Model(_args("cd_kld"), size_z=M.FIX["size_z"]).to(dev)


@pytest.mark.parametrize("n,m,Z", M.GAUSS_SHAPES)
def test_mmd_against_golden(net, dev, gold, n, m, Z):
    a, b = M.gauss_inputs(n, m, Z)
    got = net.mmd_loss(a.to(dev), b.to(dev))
    check(WORST, "mmd", f"mmd {n}x{m}x{Z}", got, M.mmd(a, b), gold[f"gauss/{n}x{m}x{Z}/mmd"], F_FWD)
    K = net.compute_kernel(a.to(dev), b.to(dev))
    check(WORST, "mmd", f"compute_kernel {n}x{m}x{Z}", K, M.gauss(a, b), gold[f"gauss/{n}x{m}x{Z}/K"], F_FWD)


# ---------------- heads + loss mix with the stub decoder ----------------

def _args(combo, **kw):
    loss, dist, opts = M.COMBOS[combo]
    return types.SimpleNamespace(loss=loss, distribution_loss=dist, loss_opts=opts, **{**M.KEY_ARGS, **kw})


class StubDecoder(torch.nn.Module):
    """tests/vrcmodel_ref.py's linear stub on the device."""

    def __init__(self, stub, shared, dev):
        super().__init__()
        self.stub, self.shared = [(b.to(dev), S.to(dev)) for b, S in stub], shared

    def forward(self, code, x):
        return M.stub_decoder(self.stub, code, self.shared)


class CountCalls:
    """Wraps calc_cd / calc_dcd of models.vrcnet: counts the calls and logs each call's NN indices."""

    def __init__(self, monkeypatch):
        import models.vrcnet as mv
        from ured_hip import nn as unn
        self.calls = []
        for name in ("calc_cd", "calc_dcd"):
            fn = getattr(mv, name)

            def wrapped(cloud, gt, *a, _fn=fn, **k):
                _, _, i1, i2 = unn.nn_dense(gt, cloud.detach())
                self.calls.append((i1.cpu().long(), i2.cpu().long()))
                return _fn(cloud, gt, *a, **k)
            monkeypatch.setattr(mv, name, wrapped)


def _stub_model(dev, combo, shared):
    from models.vrcnet import Model
    P, x, gt, noise, stub = M.fixture()
    m = Model(_args(combo), size_z=M.FIX["size_z"])
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected and all(k.startswith("decoder.") for k in missing)
    m.decoder = StubDecoder(stub, shared, dev)
    return m.to(dev), P, x, gt, noise


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("combo", list(M.COMBOS))
def test_heads_and_mix_with_stub_decoder(V, dev, refs, gold, monkeypatch, combo, shared):
    r64, r32 = refs[combo, shared, torch.float64], refs[combo, shared, torch.float32]
    what = combo + (" shared" if shared else "")
    m, P, x, gt, noise = _stub_model(dev, combo, shared)
    counter = CountCalls(monkeypatch)

    def once():
        m.zero_grad(set_to_none=True)
        del counter.calls[:]
        m.decisions = {}
        xg = x.to(dev).requires_grad_(True)
        fine, loss4, total, none = m(xg, gt.to(dev), is_training=True, alpha=M.ALPHA, noise=[t.to(dev) for t in noise])
        rec = m.decisions
        del m.decisions
        total.backward()
        g = {k: p.grad for k, p in m.named_parameters()}
        g["x"] = xg.grad
        return fine, loss4, total, none, rec, g

    fine, loss4, total, none, rec, g = once()
    assert none is None
    assert len(counter.calls) == (3 if shared else 4)
    assert torch.equal(rec["y_fps"].cpu().long(), r64["y_fps"])
    names = [n for n in M.CLOUDS if not (shared and n == "fine")]
    for name, (i1, i2) in zip(names, counter.calls):
        assert torch.equal(i1, r64["dec"].idx[f"{name}.idx1"]) and torch.equal(i2, r64["dec"].idx[f"{name}.idx2"]), name
    for k, got in (("feat", rec["feat"]), ("dl_rec", rec["dl_rec"]), ("dl_g", rec["dl_g"]), ("loss4", loss4), ("total", total),
                   ("fine", fine)):
        check(WORST, "model_fwd", f"{what} {k}", got, r32[k], r64[k], F_FWD)
    tag = combo + ("/shared" if shared else "")
    assert abs(float(total) - float(gold[f"{tag}/total"])) <= 1e-4 * abs(float(gold[f"{tag}/total"]))     # the file itself is read
    assert set(g) == set(r64["grads"])
    for k in r64["grads"]:
        check(WORST, "model_bwd", f"{what} grad {k}", g[k], r32["grads"][k], r64["grads"][k], F_GRAD)
    again = once()
    assert torch.equal(total, again[2]) and all(torch.equal(g[k], again[5][k]) for k in g), "two runs differ"


# ---------------- the whole Model, real decoder ----------------

WHOLE = dict(layers="1,1,1,1", knn_list="4,8", eval_emd=True, num_fps=32, num_points=32, num_coarse=16, num_coarse_raw=40, pk=4,
             local_folding=True, points_label=True, pts_num=[64, 32, 16, 8])
SIZE_Z = 16


def _whole(dev, loss, seed=0):
    from models.vrcnet import Model
    opts = {"alpha": 40, "lambda": 0.5} if loss == "dcd" else None
    torch.manual_seed(seed)
    m = Model(types.SimpleNamespace(loss=loss, distribution_loss="KLD", loss_opts=opts, **WHOLE), size_z=SIZE_Z)
    return m.to(dev).eval()                            # eval(): the decoder's dropout off; is_training is forward's own flag


def _clouds(dev, B=2):
    x = R.make_points(11, B, 24).transpose(1, 2).contiguous().to(dev) * 0.5
    gt = (R.make_points(12, B, 32) * 0.5).to(dev)
    return x, gt


def _noise(dev, B=2, count=2):
    g = torch.Generator().manual_seed(3)
    return [torch.randn(B, SIZE_Z, generator=g).to(dev) for _ in range(count)]


@pytest.mark.parametrize("loss", ["cd", "dcd", "emd"])
def test_model_training_wiring(V, dev, loss):
    from chamfer3D.model_utils import calc_cd, calc_dcd, calc_emd
    from ured_hip.group import GroupFn, fps
    m = _whole(dev, loss)
    x, gt = _clouds(dev)
    B, alpha = x.shape[0], 0.5
    noise = _noise(dev)

    def once(nz):
        m.zero_grad(set_to_none=True)
        fine, loss4, total, none = m(x, gt, is_training=True, alpha=alpha, noise=nz)
        total.backward()
        return fine, loss4, total, none, {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}

    fine, loss4, total, none, grads = once(noise)
    assert none is None and fine.shape == (2 * B, 32, 3) and loss4.shape == (2 * B,)
    with torch.no_grad():
        idx = fps(gt, 24, start=torch.zeros(B, dtype=torch.int32, device=dev))
        y = GroupFn.apply(None, None, gt, idx.unsqueeze(2).contiguous()).view(B, 24, 3).transpose(1, 2)
        feat = m.encoder(torch.cat((x, y), 0).contiguous())
        fx = torch.relu(feat[:B])
        z, kr, kg = V.LatentFn.apply(m.posterior_infer2(m.posterior_infer1(fx)), m.prior_infer(feat[B:]), noise[0], noise[1])
        c_raw, c_high, coarse, f = (c.transpose(1, 2).contiguous() for c in m.decoder(fx.repeat(2, 1) + m.generator(z), x.repeat(2, 1, 1)))
        g2 = gt.repeat(2, 1, 1)
        if loss == "dcd":
            l = [calc_dcd(c, g2, alpha=80 if i == 0 else 40, n_lambda=0.5)[0] for i, c in enumerate((c_raw, c_high, coarse, f))]
        else:
            l = [calc_cd(c, g2)[0] for c in (c_raw, c_high, coarse)] + [calc_emd(f, g2)[0] if loss == "emd" else calc_cd(f, g2)[0]]
        want = float(l[0].mean() * 10 + l[1].mean() * 0.5 + l[2].mean() + l[3].mean() * alpha + (kr.mean() + kg.mean()) * 20)
    got = float(total.detach())
    assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), (got, want)
    assert torch.allclose(loss4.detach(), l[3], rtol=0, atol=2e-6) and torch.equal(fine.detach(), f)
    none_set = sorted(k for k, v in grads.items() if v is None)
    assert none_set == sorted(f"decoder.conv_s{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")), none_set
    assert all(bool(torch.isfinite(v).all()) for v in grads.values() if v is not None)
    again = once(noise)
    assert torch.equal(total, again[2]) and all(v is None or torch.equal(v, again[4][k]) for k, v in grads.items()), "two runs differ"
    free = once(None)                                  # noise=None: torch.randn on the input's device
    assert bool(torch.isfinite(free[2]))
    with pytest.raises(ValueError, match="alpha"):
        m(x, gt, is_training=True)
    with pytest.raises(ValueError, match="fewer tensors"):
        m(x, gt, is_training=True, alpha=alpha, noise=noise[:1])


def test_model_evaluation_and_state_dict(V, dev):
    from models.vrcnet import Model
    m = _whole(dev, "dcd")
    src = _whole(dev, "dcd", seed=5)                   # seed-made weights, every key of the reference's layout
    sd = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())
    x, gt = _clouds(dev)
    zeros = [torch.zeros(2, SIZE_Z, device=dev)]
    with torch.no_grad():
        res = m(x, gt, is_training=False, noise=zeros)
        res2 = m(x, gt, is_training=False, test_emd=False, noise=zeros)
        res3 = m(x, gt, is_training=False, noise=None)
    assert list(res) == ["out1", "out2", "emd", "dcd", "cd_t", "f1"]
    assert res["out1"].shape == (2, 40, 3) and res["out2"].shape == (2, 32, 3)
    assert res["emd"].shape == (2,) and res["dcd"].shape == (2,) and res["cd_t"].shape == (2,) and res["f1"].shape == (2,)
    assert res2["emd"].shape == (1,) and float(res2["emd"]) == 1.0
    assert torch.equal(res["out2"], res2["out2"]), "zeros as noise must give a repeatable prediction"
    assert all(bool(torch.isfinite(v).all()) for v in list(res.values()) + list(res3.values()))


def test_five_adam_steps(V, dev):
    m = _whole(dev, "dcd", seed=1).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    x, gt = _clouds(dev)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        _, _, total, _ = m(x, gt, is_training=True, alpha=0.5)
        total.backward()
        opt.step()
        losses.append(float(total.detach()))
    assert all(np.isfinite(losses)), losses
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
