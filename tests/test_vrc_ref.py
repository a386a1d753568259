"""tests/vrc_ref.py (the float64 restatement the GPU tests of VRCNet's encoder compare against) pinned to
the reference's own modules through tests/golden/vrcnet.npz, and the CPU-side checks of
models/vrcnet.py: state_dict keys and shapes, and argument validation before any device work."""
import os

import numpy as np
import pytest
import torch

import vrc_ref as R
from chain_ref import MASK_CAP
from conftest import GOLDEN

REL = 1e-9


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "vrcnet.npz"))


@pytest.fixture(scope="module")
def runs():
    return {(n, d): R.run_fixture(n, d) for n in ("sa", "sk", "unit", "enc", "lrb") for d in (torch.float64, torch.float32)}


def _close(what, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{what:60s} err {err:.3e} max {scale:.3e}")
    assert err <= REL * scale, f"{what}: {err:.3e} > {REL} x {scale:.3e}"


@pytest.mark.parametrize("name", ["sa", "sk", "unit", "enc", "lrb"])
def test_restatement_matches_the_reference(gold, runs, name):
    assert int(gold["seed"]) == R.GOLDEN_SEED
    res = runs[name, torch.float64]
    _close(f"{name} out", res["out"], gold[f"{name}/out"])
    keys = [k[len(name) + 3:] for k in gold.files if k.startswith(f"{name}/g/")]
    assert set(keys) == set(res["grads"]), set(keys) ^ set(res["grads"])
    for k in keys:
        _close(f"{name} grad {k}", R.grad_sub(res["grads"][k]), gold[f"{name}/g/{k}"])


def test_decision_indices_match_the_reference(gold, runs):
    for name in ("sa", "sk"):
        _, _, idxs, _ = R.fixture(name)
        for i, idx in enumerate(idxs):
            assert np.array_equal(idx.numpy(), gold[f"{name}/idx{i}"])
    dec = runs["enc", torch.float64]["dec"]
    for lv in (1, 2, 3):
        assert np.array_equal(dec.idx[f"fps{lv}"].numpy(), gold[f"enc/fps{lv}"])
    for lv in (0, 1, 2):
        assert np.array_equal(dec.idx[f"three_nn{lv}"].numpy(), gold[f"enc/three_nn{lv}"])


def test_geometric_margins(runs):
    """Every geometric decision of the golden seed is at least GEO_MARGIN from a flip, so float32 kernels
    make the decisions float64 makes."""
    for dtype in (torch.float64, torch.float32):
        dec = runs["enc", dtype]["dec"]
        names = [k for k in dec.margin if k.startswith(("knn", "fps", "pn_idx", "three_nn"))]
        assert len(names) == 4 * len(R.ENC["k"]) + 3 + 3 + 3
        for k in names:
            assert dec.margin[k] >= R.GEO_MARGIN * (1 if dtype == torch.float64 else 0.99), (k, dec.margin[k])
    d64, d32 = runs["enc", torch.float64]["dec"], runs["enc", torch.float32]["dec"]
    for k in d64.idx:
        if not k.startswith(("slot", "win")):
            assert torch.equal(d64.idx[k], d32.idx[k]), k


@pytest.mark.parametrize("name", ["sa", "sk", "unit", "enc"])
def test_float32_flips_few_decisions(runs, name):
    """The condition the GPU tests rely on: float32 rounding alone flips at most MASK_CAP of a layer's
    ReLU masks, pool slots and max winners."""
    d64, d32 = runs[name, torch.float64]["dec"], runs[name, torch.float32]["dec"]
    assert set(d64.mask) == set(d32.mask)
    for k in d64.mask:
        diff, n = int((d64.mask[k] != d32.mask[k]).sum()), d64.mask[k].numel()
        assert diff <= MASK_CAP * n, (k, diff, n)
    for k in d64.idx:
        if k.startswith(("slot", "win")):
            diff, n = int((d64.idx[k] != d32.idx[k]).sum()), d64.idx[k].numel()
            assert diff <= MASK_CAP * n, (k, diff, n)


def test_modules_construct_with_the_reference_state_dict():
    from models import vrcnet as M
    S, U, E = R.SA, R.UNIT, R.ENC
    cases = [
        (M.SA_module(S["in_planes"], S["rel"], S["mid"], S["out_planes"], S["share"], S["k"]), R.fixture("sa")[0]),
        (M.SK_SA_module(S["in_planes"], S["rel"], S["mid"], S["out_planes"], S["share"], R.SK["k"]), R.fixture("sk")[0]),
        (M.SKN_Res_unit(U["input_size"], U["output_size"], U["k"], U["layers"]), R.fixture("unit")[0]),
        (M.SA_SKN_Res_encoder(E["C_in"], E["k"], E["pk"], E["output_size"], E["layers"], E["pts_num"]), R.fixture("enc")[0]),
    ]
    for mod, Pr in cases:
        sd = mod.state_dict()
        assert list(sd) == list(Pr)
        assert all(sd[k].shape == Pr[k].shape for k in sd)
        mod.load_state_dict(Pr, strict=True)
    assert cases[0][0].conv1.weight.dim() == 4
    lb = M.Linear_ResBlock(64, 16)
    assert list(lb.state_dict()) == [f"{n}.{p}" for n in ("conv1", "conv2", "conv_res") for p in ("weight", "bias")]
    assert lb(torch.zeros(2, 64)).shape == (2, 16)
    # torch's default initialisation draws the same numbers as the reference's constructors
    torch.manual_seed(R.GOLDEN_SEED)
    fresh = M.SA_SKN_Res_encoder(E["C_in"], E["k"], E["pk"], E["output_size"], E["layers"], E["pts_num"]).state_dict()
    assert all(torch.equal(fresh[k], v) for k, v in cases[3][1].items())


def test_linear_resblock_matches_the_reference(gold):
    """Plain torch, so the module itself is pinned on the CPU: the reference's in-place ReLU makes conv_res
    read relu(feature); the input here has negative entries, and the caller's tensor stays as it was."""
    from models import vrcnet as M
    Pr, x, _, cot = R.fixture("lrb")
    mod = M.Linear_ResBlock(R.LRB["input_size"], R.LRB["output_size"])
    mod.load_state_dict(Pr, strict=True)
    mod = mod.double()
    xin = x.double().requires_grad_(True)
    keep = xin.detach().clone()
    assert bool((keep < 0).any())
    out = mod(xin)
    assert torch.equal(xin.detach(), keep)
    _close("Linear_ResBlock out", out.detach(), gold["lrb/out"])
    (out * cot).sum().backward()
    _close("Linear_ResBlock dx", R.grad_sub(xin.grad), gold["lrb/g/in0"])
    for k, p in mod.named_parameters():
        _close(f"Linear_ResBlock d{k}", R.grad_sub(p.grad), gold[f"lrb/g/{k}"])
    with torch.no_grad():                              # conv_res on the raw input would differ visibly
        raw, rect = mod.conv_res(keep), mod.conv_res(keep.clamp(min=0))
    assert float((raw - rect).abs().max()) > 1e-2


def test_bad_arguments_raise_before_device_work():
    from models import vrcnet as M
    from ured_hip.vrc import EdgePoolFn, SaFn, UnpoolFn
    with pytest.raises(ValueError, match="share_planes"):
        M.SA_module(16, 4, 12, 16, share_planes=8, k=4)
    with pytest.raises(ValueError, match="outside"):
        M.SA_module(16, 4, 16, 16, share_planes=8, k=33)
    sam = M.SA_module(16, 4, 16, 16, share_planes=8, k=4)
    x = torch.zeros(2 * 3, 16)
    with pytest.raises(ValueError, match="exceeds the cloud"):
        sam.forward_rows(x, torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(TypeError, match="int32"):
        sam.forward_rows(torch.zeros(2 * 8, 16), torch.zeros(2, 8, 4, dtype=torch.int64))
    P = torch.zeros(2 * 8, 2 * 4 + 16)
    Wa, Wb, bb = torch.zeros(2, 4 * 5), torch.zeros(4 * 2, 2), torch.zeros(4 * 2)
    with pytest.raises(TypeError, match="int32"):
        SaFn.apply(P, torch.zeros(2, 8, 4, dtype=torch.int64), Wa, Wb, bb, 4, 16, 8)
    with pytest.raises(ValueError, match="exceeds the cloud"):
        SaFn.apply(torch.zeros(2 * 3, 24), torch.zeros(2, 3, 4, dtype=torch.int32), Wa, Wb, bb, 4, 16, 8)
    with pytest.raises(ValueError, match="must divide"):
        SaFn.apply(P, torch.zeros(2, 8, 4, dtype=torch.int32), Wa, Wb, bb, 4, 16, 5)
    with pytest.raises(ValueError, match="outside"):
        SaFn.apply(torch.zeros(40, 24), torch.zeros(1, 40, 33, dtype=torch.int32), Wa, Wb, bb, 4, 16, 8)
    with pytest.raises(ValueError, match="pk"):
        EdgePoolFn.apply(torch.zeros(1, 40, 4), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 33, dtype=torch.int32))
    with pytest.raises(TypeError, match="int32"):
        UnpoolFn.apply(torch.zeros(1, 4, 4), torch.zeros(1, 8, 3, dtype=torch.int64), torch.zeros(1, 8, 3), None)
    # with valid arguments the first thing that fails on this machine is the device requirement
    with pytest.raises(RuntimeError, match="MI355X"):
        SaFn.apply(P, torch.zeros(2, 8, 4, dtype=torch.int32), Wa, Wb, bb, 4, 16, 8)


def test_c_entry_points_validate_before_device_work(built):
    from ured_hip import _lib
    import ured_hip.vrc  # noqa: F401  (binds the entry points)
    with pytest.raises(_lib.UredError, match="exceeds the cloud"):
        _lib.call("ured_vrc_sa_fwd", None, None, None, None, None, 1, 3, 4, 4, 16, 2, None, None, None, None)
    with pytest.raises(_lib.UredError, match="must divide"):
        _lib.call("ured_vrc_sa_fwd", None, None, None, None, None, 1, 8, 4, 4, 16, 3, None, None, None, None)
    with pytest.raises(_lib.UredError, match="k 33"):
        _lib.call("ured_vrc_sa_fwd", None, None, None, None, None, 1, 64, 33, 4, 16, 2, None, None, None, None)
    with pytest.raises(_lib.UredError, match="pk 33"):
        _lib.call("ured_vrc_pool_fwd", None, None, None, 1, 64, 8, 33, 4, None, None, None)
    with pytest.raises(_lib.UredError, match="null pointer"):
        _lib.call("ured_vrc_unpool_fwd", None, None, None, None, 1, 8, 4, 3, 4, 0, None, None)
    with pytest.raises(_lib.UredError, match="m 5"):
        _lib.call("ured_vrc_sk_mean_fwd", None, None, None, None, 5, 1, 8, 4, None, None)
