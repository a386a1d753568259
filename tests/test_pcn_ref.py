"""CPU checks of the PCN work: tests/pcn_ref.py (the restatement that tests/test_pcn_gpu.py compares
the GPU with) is pinned to tests/golden/pcn.npz, the reference's own PCN_encoder / PCN_decoder in
float64; gen_grid_up equals the reference's; the modules construct with the reference's state_dict
keys and shapes and refuse bad arguments without a GPU; and, for the restatement alone, plain fp32
rounding flips no more ReLU / pool-winner decisions than the cap the GPU test puts on the GPU.
"""
import os
import types

import numpy as np
import pytest
import torch

import pcn_ref as R
from chain_ref import MASK_CAP
from conftest import GOLDEN

PIN = 1e-9


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "pcn.npz")))


def _pin(got, want, what):
    got, want = torch.as_tensor(got).detach().double(), torch.from_numpy(np.ascontiguousarray(want)).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    assert err <= PIN * want.abs().max().item(), f"{what}: {err:.3e} off the reference"


def test_restatement_pinned_to_golden(gold):
    seed = int(gold["seed"])
    assert seed == R.GOLDEN_SEED
    B, N, nc, scale = (R.SHAPE[k] for k in ("B", "N", "num_coarse", "scale"))
    P = R.make_params(seed, nc)
    r = R.run(P, R.make_input(seed, B, N), nc, scale, cot=R.cotangents(seed, B, nc, nc * scale))
    for k in ("feat", "coarse", "fine"):
        _pin(r[k], gold[k], k)
    for k in R.ENC_KEYS + R.DEC_KEYS:
        _pin(R.grad_sub(r["grads"][k]), gold["g/" + k], "grad " + k)


@pytest.mark.parametrize("ratio", [1, 2, 4, 8, 16])
def test_gen_grid_up(gold, built, ratio):
    from chamfer3D.model_utils import gen_grid_up
    g = gen_grid_up(ratio, 0.05)
    assert g.dtype == torch.float32 and g.is_contiguous()
    assert torch.equal(g, torch.from_numpy(gold[f"grid/{ratio}"]))
    assert torch.equal(g, R.gen_grid_up(ratio, 0.05))


def _args(loss="dcd", num_points=64):
    return types.SimpleNamespace(num_points=num_points, loss=loss, eval_emd=False, loss_opts={"alpha": 200, "lambda": 0.5})


def test_state_dict_keys_and_shapes(built):
    from models.pcn import Model
    m = Model(_args(), num_coarse=16)
    P = R.make_params(3, 16)
    sd = m.state_dict()
    assert list(sd) == R.ENC_KEYS + R.DEC_KEYS                     # grid is a plain attribute
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in P.items()}
    assert tuple(sd["encoder.conv3.weight"].shape) == (512, 512, 1)
    assert tuple(sd["decoder.conv1.weight"].shape) == (512, 1029, 1)
    m.load_state_dict(P, strict=True)
    assert tuple(m.decoder.grid.shape) == (2, 4) and not isinstance(m.decoder.grid, torch.nn.Parameter)
    assert "decoder.grid" not in dict(m.named_buffers())


def test_argument_validation(built):
    from models.pcn import PCN_decoder, PCN_encoder, Model
    with pytest.raises(ValueError, match="power of two"):
        PCN_decoder(16, 48, 3, 1029)
    with pytest.raises(ValueError, match="power of two"):
        Model(_args(num_points=96), num_coarse=16)
    with pytest.raises(ValueError, match="exceeds"):
        PCN_decoder(4, 128, 32, 1029)
    m = Model(_args(), num_coarse=16)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 3, 8), torch.zeros(1, 64, 3), alpha=0.5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        PCN_encoder()(torch.zeros(1, 3, 8))
    from ured_hip import _lib
    with pytest.raises(_lib.UredError, match="scale"):
        _lib.call("ured_pcn_fold_bwd", None, None, 1, 4, 17, 512, 32, None, None, None)
    with pytest.raises(_lib.UredError, match="bad sizes"):
        _lib.call("ured_pcn_fold_fwd", None, None, None, 1, 0, 2, 512, None, None)
    _lib.call("ured_pcn_relu", None, None, 0, None, None)           # succeeds: the error message is empty again
    assert _lib.lib().ured_last_error() == b""


@pytest.mark.parametrize("seed", [R.GOLDEN_SEED, 2, 3, 4])
def test_fp32_decisions_of_the_restatement(seed):
    """The restatement alone, float32 against float64, at the shape of the GPU test: fp32 rounding
    flips at most MASK_CAP of a layer's ReLU decisions and pool winners."""
    B, N, nc, scale = (R.SHAPE[k] for k in ("B", "N", "num_coarse", "scale"))
    P, x = R.make_params(seed, nc), R.make_input(seed, B, N)
    with torch.no_grad():
        r64, r32 = R.run(P, x, nc, scale), R.run(P, x, nc, scale, dtype=torch.float32)
    for k, (n, tot) in R.differing_decisions(r64["pre"], r32["pre"]).items():
        print(f"seed {seed} {k}: {n} of {tot} decisions differ")
        assert n <= MASK_CAP * tot, f"seed {seed} {k}: {n} of {tot} fp32 decisions differ from float64"
