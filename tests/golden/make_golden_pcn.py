"""Writes tests/golden/pcn.npz: the seed and the float64 outputs and gradients of the reference's
PCN_encoder / PCN_decoder (Density_aware_Chamfer_Distance/models/pcn.py:13-71), and its gen_grid_up
(utils/model_utils.py:251-264). Run on a machine that has the reference tree (never on the GPU box):

    python tests/golden/make_golden_pcn.py <reference root>

The two classes and gen_grid_up are lifted from the reference's source with `ast` (utils/model_utils.py
imports CUDA-only extensions and cannot be imported whole); while they run, Tensor.cuda returns the
tensor itself. Only data goes into the npz: the seed, coarse, fine, the encoder feature and at most
GRAD_CAP strided elements of every parameter gradient under fixed cotangents on (coarse, fine).
Weights and inputs are not stored: tests/pcn_ref.py regenerates them (make_params draws what the
reference's own modules draw under the same seed, asserted here).
"""
import ast
import math
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pcn_ref as R  # noqa: E402


def lift(ref, path, names, ns):
    tree = ast.parse(open(os.path.join(ref, path)).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in body} == set(names), (path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)


class no_cuda:
    """Tensor.cuda returns the tensor itself."""

    def __enter__(self):
        self.saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda t, *a, **k: t

    def __exit__(self, *exc):
        torch.Tensor.cuda = self.saved


def main(ref):
    ns = {"torch": torch, "nn": nn, "F": F, "math": math, "np": np}
    lift(ref, "Density_aware_Chamfer_Distance/utils/model_utils.py", ["gen_grid_up"], ns)
    lift(ref, "Density_aware_Chamfer_Distance/models/pcn.py", ["PCN_encoder", "PCN_decoder"], ns)
    out = {"seed": np.array(R.GOLDEN_SEED)}
    for r in (1, 2, 4, 8, 16):
        out[f"grid/{r}"] = ns["gen_grid_up"](r, 0.05).numpy()
    B, N, nc, scale = (R.SHAPE[k] for k in ("B", "N", "num_coarse", "scale"))
    with no_cuda():
        torch.manual_seed(R.GOLDEN_SEED)
        enc = ns["PCN_encoder"]()
        dec = ns["PCN_decoder"](nc, nc * scale, scale, 1029)
        sd = {f"encoder.{k}": v for k, v in enc.state_dict().items()}
        sd.update({f"decoder.{k}": v for k, v in dec.state_dict().items()})
        P = R.make_params(R.GOLDEN_SEED, nc)
        assert list(sd) == R.ENC_KEYS + R.DEC_KEYS and all(torch.equal(sd[k], P[k]) for k in sd)
        enc, dec = enc.double(), dec.double()
        dec.grid = dec.grid.double()
        x = R.make_input(R.GOLDEN_SEED, B, N).double()
        feat = enc(x)
        coarse, fine = dec(feat)
        cc, cf = R.cotangents(R.GOLDEN_SEED, B, nc, nc * scale)
        ((coarse * cc).sum() + (fine * cf).sum()).backward()
    out["feat"], out["coarse"], out["fine"] = feat.detach().numpy(), coarse.detach().numpy(), fine.detach().numpy()
    for pre, mod in (("encoder", enc), ("decoder", dec)):
        for k, p in mod.named_parameters():
            out[f"g/{pre}.{k}"] = R.grad_sub(p.grad).numpy()
    np.savez_compressed(os.path.join(HERE, "pcn.npz"), **out)
    print("wrote pcn.npz", sum(v.nbytes for v in out.values()), "bytes raw")


if __name__ == "__main__":
    main(sys.argv[1])
