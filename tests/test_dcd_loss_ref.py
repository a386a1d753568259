"""CPU checks of the DCD training loss: tests/dcd_loss_ref.py (the float64 restatement that
tests/test_dcd_loss_gpu.py compares the GPU with) equals oracle/dcd_ref.calc_dcd and
tests/golden/dcd_loss.npz, the reference's own calc_dcd and its autograd gradient through the
float64 distChamfer; and the library refuses bad arguments before any device work.
"""
import os

import numpy as np
import pytest
import torch

import dcd_loss_ref as R
from conftest import GOLDEN
from oracle import dcd_ref, nn_ref

TOL = 2e-6       # tests/test_pairs_gpu.py: fp32 means of ~1e3 terms in another order
# The reference runs the tail (exp, weights, mean and their autograd) in float32: a chain of about
# ten roundings of 6e-8 each per gradient term and up to `count` terms per point; 2e-5 of the
# largest gradient entry is the gradient floor of tests/tol_check.py.
F_GRAD = 2e-5


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "dcd_loss.npz")))


@pytest.fixture(scope="module")
def cases(gold):
    out = {}
    for name, (seed, b, n_x, n_gt) in R.GOLDEN_CASES.items():
        assert int(gold[name + "/seed"]) == seed
        x, gt = R.make_inputs(seed, b, n_x, n_gt)
        out[name] = (x, gt, nn_ref.nn_fwd(gt, x))
    return out


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_float64_and_fp32_decisions_agree(cases, name):
    """The condition under which the restatement (the oracle's decisions) and the reference (the
    float64 distChamfer's) differentiate the same function."""
    x, gt, o = cases[name]
    _, _, i1, i2 = nn_ref.dist_chamfer(torch.from_numpy(gt), torch.from_numpy(x))
    assert (i1.numpy() == o[2]).all() and (i2.numpy() == o[3]).all()


@pytest.mark.parametrize("alpha,lam,nr", R.PARAMS)
@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_restatement_matches_oracle_and_reference(gold, cases, name, alpha, lam, nr):
    x, gt, o = cases[name]
    b = x.shape[0]
    out, grads = R.run(x, gt, o[2], o[3], alpha, lam, nr, cot={"loss": R.cotangent(b)})
    tag = f"{name}/{R.param_tag(alpha, lam, nr)}"
    ol, op, ot = dcd_ref.calc_dcd(x, gt, alpha=alpha, n_lambda=lam, non_reg=nr)
    for key, orc in (("loss", ol), ("cd_p", op), ("cd_t", ot)):
        got = out[key].numpy()
        np.testing.assert_allclose(got, orc, rtol=0, atol=TOL, err_msg=f"{tag} {key} vs oracle")
        np.testing.assert_allclose(got, gold[f"{tag}/{key}"], rtol=0, atol=TOL, err_msg=f"{tag} {key} vs reference")
    for key, g in (("gx", grads["x"]), ("ggt", grads["gt"])):
        want = gold[f"{tag}/{key}"].astype(np.float64)
        err = np.abs(g.numpy() - want).max()
        print(f"{tag} {key}: err {err:.3e} of max {np.abs(want).max():.3e}")
        assert err <= F_GRAD * np.abs(want).max(), f"{tag} {key}: {err:.3e} off the reference's autograd gradient"


def test_fp32_restatement_is_close():
    """ref32 of the GPU tests: the same restatement in float32 stays within 1e-5 of float64."""
    x, gt = R.make_inputs(3, 2, 100, 140)
    o = nn_ref.nn_fwd(gt, x)
    a, _ = R.run(x, gt, o[2], o[3], 200, 0.5)
    c, _ = R.run(x, gt, o[2], o[3], 200, 0.5, dtype=torch.float32)
    assert (a["loss"] - c["loss"].double()).abs().max().item() <= 1e-5


def test_arguments_refused_before_device_work(built):
    from ured_hip import _lib
    with pytest.raises(_lib.UredError, match="exceeds"):
        _lib.call("ured_dcd_loss_fwd", None, None, None, None, 1, 9000, 9000, 1000.0, 1.0, 1.0, 1.0,
                  None, None, None, None, None, None)
    with pytest.raises(_lib.UredError, match="lambda"):
        _lib.call("ured_dcd_loss_fwd", None, None, None, None, 1, 4, 4, 1000.0, -0.5, 1.0, 1.0,
                  None, None, None, None, None, None)
    with pytest.raises(_lib.UredError, match="bad sizes"):
        _lib.call("ured_dcd_loss_bwd", None, None, None, None, None, None, None, None, None, 1, 0, 4,
                  None, None, None)
    import ured_hip.dcd as D
    with pytest.raises(RuntimeError, match="MI355X only"):
        D.dcd_loss(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    # a call that succeeds (b = 0: no device work) leaves the thread's error message empty again
    _lib.call("ured_dcd_loss_fwd", None, None, None, None, 0, 4, 4, 1000.0, 1.0, 1.0, 1.0,
              None, None, None, None, None, None)
    assert _lib.lib().ured_last_error() == b""
