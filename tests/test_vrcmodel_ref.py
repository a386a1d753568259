"""CPU checks of VRCNet's Model: tests/vrcmodel_ref.py (the restatement that tests/test_vrcmodel_gpu.py compares
the GPU with) is pinned to tests/golden/vrcmodel.npz, the reference's own Model in float64 with a stub decoder;
its latent head equals torch.distributions computed here; the seed rule holds; models.vrcnet.Model constructs
with the reference's state_dict keys and shapes; and the argument checks raise without a device.
"""
import os
import types

import numpy as np
import pytest
import torch

import vrc_ref as R
import vrcmodel_ref as M
from conftest import GOLDEN

PIN = 1e-9


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "vrcmodel.npz")))


def _pin(got, want, what):
    got, want = torch.as_tensor(got).detach().double(), torch.as_tensor(np.asarray(want)).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    assert err <= PIN * want.abs().max().item(), f"{what}: {err:.3e} off the reference"


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("combo", list(M.COMBOS))
def test_restatement_pinned_to_golden(gold, combo, shared):
    assert int(gold["seed"]) == M.GOLDEN_SEED
    tag = combo + ("/shared" if shared else "")
    r = M.run_fixture(combo, torch.float64, shared)
    assert np.array_equal(r["y_fps"].numpy(), gold[f"{tag}/y_fps"])
    for name in M.CLOUDS:
        if shared and name == "fine":
            continue                                   # the restatement makes one pick for the shared cloud
        for i in ("idx1", "idx2"):
            assert np.array_equal(r["dec"].idx[f"{name}.{i}"].numpy(), gold[f"{tag}/{i}/{name}"]), (name, i)
    if shared:
        for i in ("idx1", "idx2"):
            assert np.array_equal(gold[f"{tag}/{i}/fine"], gold[f"{tag}/{i}/coarse"])
    for k in ("feat", "dl_rec", "dl_g", "loss4", "total"):
        _pin(r[k], gold[f"{tag}/{k}"], f"{tag} {k}")
    for k, g in r["grads"].items():
        _pin(M.grad_sub(g), gold[f"{tag}/g/{k}"], f"{tag} grad {k}")
        assert gold[f"{tag}/g/{k}"].size <= M.GRAD_CAP


@pytest.mark.parametrize("n,m,Z", M.GAUSS_SHAPES)
def test_gauss_pinned_to_golden(gold, n, m, Z):
    a, b = (t.double() for t in M.gauss_inputs(n, m, Z))
    _pin(M.gauss(a, b), gold[f"gauss/{n}x{m}x{Z}/K"], "compute_kernel")
    _pin(M.mmd(a, b), gold[f"gauss/{n}x{m}x{Z}/mmd"], "mmd_loss")


def test_latent_equals_torch_distributions():
    """The restated samples and KL terms against Normal.rsample / kl_divergence, values and gradients."""
    import torch.distributions as D
    import torch.distributions.normal as N
    g = torch.Generator().manual_seed(5)
    B, Z = 3, 7
    oq = torch.randn(B, 2 * Z, generator=g, dtype=torch.float64).requires_grad_(True)
    op = torch.randn(B, 2 * Z, generator=g, dtype=torch.float64).requires_grad_(True)
    with torch.no_grad():
        oq[0, Z], oq[0, Z + 1], op[0, Z] = 20.0, 25.0, 20.0 + 1e-3          # on and above softplus's threshold
    eq, ep = (torch.randn(B, Z, generator=g, dtype=torch.float64) for _ in range(2))
    cz, ck = torch.randn(2 * B, Z, generator=g, dtype=torch.float64), torch.randn(2, B, Z, generator=g, dtype=torch.float64)

    def grads(z, kr, kg):
        return torch.autograd.grad((z * cz).sum() + (kr * ck[0]).sum() + (kg * ck[1]).sum(), [oq, op])

    z, kr, kg = M.latent(oq, op, eq, ep)
    q = D.Normal(oq[:, :Z], torch.nn.functional.softplus(oq[:, Z:]))
    p = D.Normal(op[:, :Z], torch.nn.functional.softplus(op[:, Z:]))
    draws = [eq, ep]
    saved = N._standard_normal
    N._standard_normal = lambda shape, dtype, device: draws.pop(0)
    try:
        zt = torch.cat((q.rsample(), p.rsample()), 0)
    finally:
        N._standard_normal = saved
    krt = D.kl_divergence(D.Normal(torch.zeros_like(p.loc), torch.ones_like(p.scale)), p)
    kgt = D.kl_divergence(D.Normal(p.loc.detach(), p.scale.detach()), q)
    for a, b, what in ((z, zt, "z"), (kr, krt, "kl_rec"), (kg, kgt, "kl_g")):
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), what
    for a, b, what in zip(grads(z, kr, kg), grads(zt, krt, kgt), ("d_oq", "d_op")):
        assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item(), what
    ze = M.latent(oq, None, eq, None)
    assert ze[1] is None and ze[2] is None and torch.equal(ze[0], z[:B])
    same = M.latent(oq, oq.detach().clone(), eq, ep)[2]
    assert float(same.detach().abs().max()) == 0.0                         # equal distributions: exactly zero


def test_seed_rule(gold):
    """The golden seed keeps every NN argmin gap of the loss heads MARGIN_MULT times the forward tolerance of its
    distance matrix and the FPS steps on gt GEO_MARGIN apart; float32 makes the same picks."""
    ratio = M.qualify(M.GOLDEN_SEED)
    print("smallest ratio", ratio)
    assert ratio is not None and ratio >= M.MARGIN_MULT
    assert abs(ratio - M.GOLDEN_RATIO) <= 0.1 * ratio and abs(float(gold["ratio"]) - M.GOLDEN_RATIO) == 0.0
    P, x, gt, noise, stub = M.fixture()
    assert R.fps_pick(gt.double(), M.FIX["n_in"])[1] >= R.GEO_MARGIN


def _args(combo="dcd_kld", **kw):
    loss, dist, opts = M.COMBOS[combo]
    return types.SimpleNamespace(loss=loss, distribution_loss=dist, loss_opts=opts, **{**M.KEY_ARGS, **kw})


def test_state_dict_keys_and_shapes(gold, built):
    from models.vrcnet import Model
    m = Model(_args(), size_z=M.FIX["size_z"])
    sd = m.state_dict()
    assert list(sd) == list(gold["keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(gold["shapes"])
    P = M.make_params(3)
    assert list(sd)[:len(P)] == list(P)
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected and all(k.startswith("decoder.") for k in missing)
    assert [n for n, _ in m.named_children()] == ["encoder", "posterior_infer1", "posterior_infer2", "prior_infer", "generator",
                                                  "decoder"]


def test_argument_validation(built):
    from models.vrcnet import Model
    from ured_hip import GaussKernelFn, LatentFn, _lib, vrc
    f = torch.zeros
    with pytest.raises(ValueError, match="halves"):
        LatentFn.apply(f(2, 5), None, f(2, 2), None)
    with pytest.raises(ValueError, match=r"Z 4097 outside"):
        LatentFn.apply(f(1, 2 * 4097), None, f(1, 4097), None)
    with pytest.raises(ValueError, match="go together"):
        LatentFn.apply(f(2, 4), f(2, 4), f(2, 2), None)
    with pytest.raises(ValueError, match="eps_p has shape"):
        LatentFn.apply(f(2, 4), f(2, 4), f(2, 2), f(2, 3))
    with pytest.raises(TypeError, match="float32"):
        LatentFn.apply(f(2, 4).double(), None, f(2, 2), None)
    with pytest.raises(RuntimeError, match="MI355X only"):
        LatentFn.apply(f(2, 4), f(2, 4), f(2, 2), f(2, 2))
    with pytest.raises(ValueError, match=r"B 65536 outside"):
        vrc.latent_check("t", 65536, 1)
    vrc.latent_check("t", 65535, 4096)                  # the largest B and Z together stay below 2^31 elements
    with pytest.raises(ValueError, match="outside"):
        GaussKernelFn.apply(f(4097, 2), f(1, 2))
    with pytest.raises(ValueError, match="y has shape"):
        GaussKernelFn.apply(f(3, 2), f(3, 4))
    with pytest.raises(RuntimeError, match="MI355X only"):
        GaussKernelFn.apply(f(3, 2), f(2, 2))
    with pytest.raises(_lib.UredError, match="Z 0 outside"):
        _lib.call("ured_vrc_latent_fwd", None, None, None, None, 1, 0, None, None, None, None)
    with pytest.raises(_lib.UredError, match="B 65536 outside"):
        _lib.call("ured_vrc_latent_bwd", None, None, None, None, None, None, None, 65536, 4, None, None, None)
    with pytest.raises(_lib.UredError, match="null pointer"):
        _lib.call("ured_vrc_latent_fwd", None, None, None, None, 2, 4, None, None, None, None)
    with pytest.raises(_lib.UredError, match="m 4097 outside"):
        _lib.call("ured_vrc_gauss_fwd", None, None, 1, 4097, 4, None, None)
    with pytest.raises(_lib.UredError, match="Z 4097 outside"):
        _lib.call("ured_vrc_gauss_bwd", None, None, None, None, 1, 1, 4097, None, None, None)
    with pytest.raises(_lib.UredError, match="null pointer"):
        _lib.call("ured_vrc_gauss_bwd", None, None, None, None, 1, 1, 1, None, None, None)
    _lib.call("ured_pcn_relu", None, None, 0, None, None)           # succeeds: the error message is empty again
    assert _lib.lib().ured_last_error() == b""
    m = Model(_args(), size_z=16)
    with pytest.raises(ValueError, match="alpha"):
        m(f(1, 3, 8), f(1, 32, 3))
    with pytest.raises(ValueError, match=r"gt must be"):
        m(f(1, 3, 8), f(2, 32, 3), alpha=0.5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(f(1, 3, 8), f(1, 32, 3), alpha=0.5)
    with pytest.raises(ValueError, match="Z 5000 outside"):
        Model(_args(), size_z=5000)
