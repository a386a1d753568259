"""Writes tests/golden/dcd_loss.npz: seeds and the outputs and gradients of the reference's
calc_dcd (Density_aware_Chamfer_Distance/utils_v2/model_utils.py:13-70) run on the reference's own
python chamfer (utils_v2/metrics/CD/chamfer_python.py: distChamfer, float64, differentiable). Run on
a machine that has the reference tree (never on the GPU box):

    python tests/golden/make_golden_dcd_loss.py <reference root>

calc_dcd and calc_cd are lifted from the reference's source with `ast` (the module imports CUDA-only
extensions and cannot be imported whole); `cd()` is distChamfer. Only data goes into the npz: the
seeds, loss / cd_p / cd_t and the gradients with respect to x and gt of sum(loss * cotangent).
Inputs are not stored: tests/dcd_loss_ref.py regenerates them (make_inputs, cotangent).

Condition asserted here and again in tests/test_dcd_loss_ref.py: the float64 distChamfer indices
equal the fp32 C oracle's (oracle/nn_ref) in both directions, so the restatement under the oracle's
decisions and the reference differentiate the same function.
"""
import ast
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), ROOT]
import dcd_loss_ref as R  # noqa: E402
from oracle import nn_ref  # noqa: E402


def lift(ref, path, names, ns):
    tree = ast.parse(open(os.path.join(ref, path)).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names), (path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)


def main(ref):
    sys.path.insert(0, os.path.join(ref, "Density_aware_Chamfer_Distance/utils_v2/metrics/CD"))
    import chamfer_python
    assert os.path.realpath(chamfer_python.__file__).startswith(os.path.realpath(ref) + "/")

    class CD:
        def __call__(self, a, b):
            return chamfer_python.distChamfer(a, b)

    ns = {"torch": torch, "cd": CD}
    lift(ref, "Density_aware_Chamfer_Distance/utils_v2/model_utils.py", ["calc_dcd", "calc_cd"], ns)
    out = {}
    for name, (seed, b, n_x, n_gt) in R.GOLDEN_CASES.items():
        x, gt = R.make_inputs(seed, b, n_x, n_gt)
        out[name + "/seed"] = np.array(seed)
        o = nn_ref.nn_fwd(gt, x)
        for alpha, lam, nr in R.PARAMS:
            xt, gtt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(gt).requires_grad_(True)
            loss, cd_p, cd_t, _, _, i1, i2 = ns["calc_dcd"](xt, gtt, alpha=alpha, n_lambda=lam, return_raw=True, non_reg=nr)
            assert (i1.numpy() == o[2]).all() and (i2.numpy() == o[3]).all(), "float64 / fp32 NN decisions differ"
            (loss * torch.from_numpy(R.cotangent(b)).float()).sum().backward()
            tag = f"{name}/{R.param_tag(alpha, lam, nr)}"
            out[tag + "/loss"], out[tag + "/cd_p"], out[tag + "/cd_t"] = (
                loss.detach().numpy(), cd_p.detach().numpy(), cd_t.detach().numpy())
            out[tag + "/gx"], out[tag + "/ggt"] = xt.grad.numpy(), gtt.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "dcd_loss.npz"), **out)
    print("wrote dcd_loss.npz", sum(v.nbytes for v in out.values()), "bytes raw")


if __name__ == "__main__":
    main(sys.argv[1])
