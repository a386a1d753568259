"""Writes tests/golden/vrcmodel.npz: the float64 training forward and gradients of the reference's Model
(Density_aware_Chamfer_Distance/models/vrcnet.py:406-539) with its decoder replaced by a linear stub. Run on a
machine that has the reference tree (never on the GPU box):

    python tests/golden/make_golden_vrcmodel.py <reference root>

Works as make_golden_vrcnet.py / make_golden_vrcdec.py do and reuses their `lift`, float64 `pn2` stand-in and
no_cuda / CpuTorch shims. Model, Linear_ResBlock, the decoder's classes and PCN_encoder are lifted from the
reference's source with `ast`. While the lifted Model runs:
  - torch.distributions.normal._standard_normal (what Normal.rsample calls) hands out the fixture's noise;
  - Tensor.chunk returns copies. The reference rectifies chunks of the encoder's output in place (the in-place
    ReLU of Linear_ResBlock), which current torch refuses on the views chunk returns; on a copy the same
    arithmetic runs and the rectified chunk is what goes on to the decoder, as it did where the reference ran;
  - `decoder` is the stub of tests/vrcmodel_ref.py (each cloud = base_i + reshape(code @ S_i)); a second variant
    returns one tensor as both coarse and fine;
  - calc_cd / calc_dcd in the lifted namespace are float64 stand-ins on the repository's own pinned restatement
    (tests/dcd_loss_ref.py, pinned to the reference's calc_dcd by tests/golden/dcd_loss.npz) with the
    nearest-neighbour picks taken from the direct squared distance; the C NN oracle (oracle/nn_ref.py, float32)
    must make the same picks (asserted);
  - for the MMD fixture, `mmd_loss2 = mmd_loss` on the lifted class (the reference defines no mmd_loss2).
Only data goes into the npz: the seed, y's FPS indices, the code handed to the decoder, dl_rec, dl_g, loss4,
total, the NN indices of the heads, at most GRAD_CAP strided elements of the gradient of every encoder / head
parameter and of x, the state_dict key list and shapes of the real, unstubbed reference Model, and
compute_kernel / mmd_loss values for a few shapes. Weights, inputs, noise and the stub are regenerated from the
seed by tests/vrcmodel_ref.py (asserted here). The seed is the first below 256 that satisfies the rule in
tests/vrcmodel_ref.py's docstring.
"""
import math
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import dcd_loss_ref  # noqa: E402
import vrcmodel_ref as M  # noqa: E402
from make_golden_vrcnet import CpuTorch, MAX_BYTES, Pn2, lift, no_cuda  # noqa: E402
from oracle import nn_ref  # noqa: E402

SEED_LIMIT = 256


class fixed_noise:
    """Normal.rsample draws from `draws` (a list, consumed in order)."""

    def __init__(self, draws):
        self.draws = list(draws)

    def __enter__(self):
        import torch.distributions.normal as N
        self.mod, self.saved = N, N._standard_normal

        def take(shape, dtype, device):
            t = self.draws.pop(0)
            assert tuple(t.shape) == tuple(shape), (t.shape, shape)
            return t.to(dtype)
        N._standard_normal = take
        return self

    def __exit__(self, *exc):
        self.mod._standard_normal = self.saved


class chunk_copies:
    """Tensor.chunk returns copies (see the module docstring)."""

    def __enter__(self):
        self.saved = torch.Tensor.chunk
        saved = self.saved
        torch.Tensor.chunk = lambda t, *a, **k: tuple(c.clone() for c in saved(t, *a, **k))

    def __exit__(self, *exc):
        torch.Tensor.chunk = self.saved


class TorchLog(CpuTorch):
    """CpuTorch whose distributions.kl_divergence logs its results."""

    def __init__(self):
        self.kl = []

        def kl_divergence(p, q):
            out = torch.distributions.kl_divergence(p, q)
            self.kl.append(out)
            return out
        self.distributions = types.SimpleNamespace(Normal=torch.distributions.Normal, kl_divergence=kl_divergence)


class Stub(nn.Module):
    def __init__(self, stub, shared):
        super().__init__()
        self.stub, self.shared, self.seen = stub, shared, []

    def forward(self, code, x):
        self.seen.append(code)
        return M.stub_decoder(self.stub, code, self.shared)


class Losses:
    """float64 calc_cd / calc_dcd with the reference's signatures and return lists; logs every call's indices."""

    def __init__(self):
        self.calls = []

    def _nn(self, x, gt):
        idx1, _, _ = M.nn_pick(gt.detach(), x.detach())
        idx2, _, _ = M.nn_pick(x.detach(), gt.detach())
        o = nn_ref.nn_fwd(gt.detach().float().numpy(), x.detach().float().numpy())
        assert (o[2] == idx1.numpy()).all() and (o[3] == idx2.numpy()).all(), "the float32 NN oracle picks differently"
        self.calls.append((idx1, idx2))
        return idx1, idx2

    def calc_cd(self, output, gt, calc_f1=False, return_raw=False, normalize=False, separate=False):
        assert not (calc_f1 or normalize or separate)
        idx1, idx2 = self._nn(output, gt)
        o = dcd_loss_ref.forward(output, gt, idx1, idx2, 1, 1)
        res = [o["cd_p"], o["cd_t"]]
        if return_raw:
            res.extend([o["dist1"], o["dist2"], idx1, idx2])
        return res

    def calc_dcd(self, x, gt, alpha=1000, n_lambda=1, return_raw=False, non_reg=False):
        idx1, idx2 = self._nn(x, gt)
        o = dcd_loss_ref.forward(x, gt, idx1, idx2, alpha, n_lambda, non_reg)
        res = [o["loss"], o["cd_p"], o["cd_t"]]
        if return_raw:
            res.extend([o["dist1"], o["dist2"], idx1, idx2])
        return res


def args_of(combo, **kw):
    loss, dist, opts = M.COMBOS[combo]
    return types.SimpleNamespace(loss=loss, distribution_loss=dist, loss_opts=opts, **M.KEY_ARGS, **kw)


def main(ref):
    seed, ratio = next((s, r) for s in range(SEED_LIMIT) for r in [M.qualify(s)] if r is not None)
    print("seed", seed, "smallest ratio", repr(ratio))
    assert seed == M.GOLDEN_SEED, f"the first qualifying seed is {seed}; tests/vrcmodel_ref.py says {M.GOLDEN_SEED}"
    assert abs(ratio - M.GOLDEN_RATIO) <= 0.1 * ratio, f"tests/vrcmodel_ref.py says {M.GOLDEN_RATIO}"
    pn2 = Pn2()
    tl = TorchLog()
    losses = Losses()
    ns = {"torch": tl, "nn": nn, "F": F, "np": np, "pn2": pn2, "math": math, "calc_cd": losses.calc_cd,
          "calc_dcd": losses.calc_dcd, "print": lambda *a, **k: None}
    lift(ref, "Density_aware_Chamfer_Distance/utils/model_utils.py",
         ["knn", "knn_point", "get_edge_features", "edge_preserve_sampling", "three_nn_upsampling", "get_graph_feature",
          "EF_expansion"], ns)
    lift(ref, "Density_aware_Chamfer_Distance/models/pcn.py", ["PCN_encoder"], ns)
    lift(ref, "Density_aware_Chamfer_Distance/models/vrcnet.py",
         ["SA_module", "SK_SA_module", "SKN_Res_unit", "SA_SKN_Res_encoder", "Linear_ResBlock", "Folding", "MSAP_SKN_decoder",
          "Model"], ns)
    Model = ns["Model"]
    Model.mmd_loss2 = Model.mmd_loss
    mmd_log = []
    mmd_ref = Model.mmd_loss

    def mmd_logged(self, x, y):
        out = mmd_ref(self, x, y)
        mmd_log.append(out)
        return out
    out = {"seed": np.array(seed), "ratio": np.array(M.GOLDEN_RATIO)}
    P, x, gt, noise, stub = M.fixture(seed)
    with no_cuda():
        torch.manual_seed(seed)
        real = Model(args_of("cd_kld"))
        sd = real.state_dict()
        out["keys"] = np.array(list(sd))
        out["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        assert all(torch.equal(sd[k], P[k]) for k in P) and list(sd)[:len(P)] == list(P)
        for combo in M.COMBOS:
            for shared in (False, True):
                tag = combo + ("/shared" if shared else "")
                torch.manual_seed(seed)
                mod = Model(args_of(combo))
                mod.decoder = Stub(stub, shared)
                mod = mod.double()
                Model.mmd_loss = Model.mmd_loss2 = mmd_logged
                xg = x.double().requires_grad_(True)
                pn2.log = {"fps": [], "three_nn": []}
                del tl.kl[:], mmd_log[:], losses.calls[:]
                with fixed_noise(noise) as fn, chunk_copies():
                    fine, loss4, total, none = mod(xg, gt.double(), is_training=True, alpha=M.ALPHA)
                Model.mmd_loss = Model.mmd_loss2 = mmd_ref
                assert none is None and len(fn.draws) == (0 if M.COMBOS[combo][1] == "MMD" else 4)
                total.backward()
                dl = mmd_log if M.COMBOS[combo][1] == "MMD" else tl.kl
                assert len(dl) == 2 and len(losses.calls) == 4 and len(pn2.log["fps"]) == 1
                out[f"{tag}/y_fps"] = pn2.log["fps"][0].numpy().astype(np.int16)
                out[f"{tag}/feat"] = mod.decoder.seen[0].detach().numpy()
                out[f"{tag}/dl_rec"], out[f"{tag}/dl_g"] = dl[0].detach().numpy(), dl[1].detach().numpy()
                out[f"{tag}/loss4"], out[f"{tag}/total"] = loss4.detach().numpy(), total.detach().numpy()
                for name, (i1, i2) in zip(M.CLOUDS, losses.calls):
                    out[f"{tag}/idx1/{name}"] = i1.numpy().astype(np.int16)
                    out[f"{tag}/idx2/{name}"] = i2.numpy().astype(np.int16)
                for k, p in mod.named_parameters():
                    assert p.grad is not None, k
                    out[f"{tag}/g/{k}"] = M.grad_sub(p.grad).numpy()
                out[f"{tag}/g/x"] = M.grad_sub(xg.grad).numpy()
                r = M.run_fixture(combo, torch.float64, shared, seed)      # the restatement, for the record
                print(tag, "total", float(total), "restated", float(r["total"]))
        for n, m, Z in M.GAUSS_SHAPES:
            a, b = (t.double() for t in M.gauss_inputs(n, m, Z))
            out[f"gauss/{n}x{m}x{Z}/K"] = real.compute_kernel(a, b).numpy()
            out[f"gauss/{n}x{m}x{Z}/mmd"] = mmd_ref(real, a, b).numpy()
    path = os.path.join(HERE, "vrcmodel.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("wrote vrcmodel.npz", size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
