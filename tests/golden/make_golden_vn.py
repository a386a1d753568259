"""Writes tests/golden/vn.npz: seeds and the float64 outputs, running statistics and gradients of the
reference's network/VN/vn_encoder.py (vn_encoder) and vn_retrieval.py (vn_retrieval). Run on a
machine that has the reference tree (never on the GPU box):

    python tests/golden/make_golden_vn.py <reference root>

The reference modules are imported from <reference root> and run in float64 on the CPU.
get_graph_feature hard-codes torch.device('cuda') for one torch.arange; while the reference runs,
torch.arange drops its `device` argument. Only data goes into the npz. Weights and inputs are not
stored: tests/vn_ref.py regenerates them from the recorded seeds (encoder_params, encoder_input,
act_case_inputs, pool_case_inputs). Of the per-point features every POINT_STRIDE-th point is stored
and of every parameter gradient at most GRAD_CAP evenly strided elements (grad_sub below), to keep
the file near the size of the other goldens; tests/test_vn_ref.py pins vn_ref.encoder to them and
the GPU test compares whole tensors with vn_ref.encoder in float64.

Seeds are searched until the conditions hold that make a GPU comparison meaningful, for the float64
restatement alone (tests/test_vn_ref.py asserts them again):
  kernel cases: every leaky-mask and pool-winner margin is at least 1e-4;
  encoders (a seed per pooling and mode): every kNN and pool-winner margin is at least 1e-4, and at most 0.1 %
    of a layer's leaky-mask decisions have a margin below 1e-4.
"""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vn_ref as R  # noqa: E402

POINT_STRIDE = 4
GRAD_CAP = 512


def grad_sub(t):
    """At most GRAD_CAP evenly strided elements of the flattened tensor."""
    flat = t.reshape(-1)
    return flat[::max(1, -(-flat.numel() // GRAD_CAP))]


class reference_run:
    """torch.arange without its device argument."""

    def __enter__(self):
        self.saved = torch.arange

        def arange(*a, **k):
            k.pop("device", None)
            return self.saved(*a, **k)
        torch.arange = arange
        return self

    def __exit__(self, *exc):
        torch.arange = self.saved


def encoder_ok(seed, pooling, training):
    P, x = R.encoder_params(seed, pooling), R.encoder_input(seed)
    with torch.no_grad():
        r = R.encoder(P, x, training, pooling)
    if min(r["knn_margin"], r["slot_margin"]) < R.MARGIN:
        return False
    if not all(float((m < R.MARGIN).double().mean()) <= 1e-3 for m in r["mask_margins"]):
        return False
    return R.encoder_same_decisions(P, x, training, pooling, r)


def main(ref_root):
    sys.path.insert(0, ref_root)
    from network.VN.vn_encoder import vn_encoder
    from network.VN.vn_retrieval import vn_retrieval
    out = {}
    act_seeds = []
    for case in R.ACT_CASES:
        def margin(seed):
            r = R.act_run(case, R.act_case_inputs(case, seed), torch.float64)
            return float(r["margin"].min())
        act_seeds.append(R.search_seed(margin))
    out["act_seeds"] = np.array(act_seeds, dtype=np.int64)
    pool_seeds = []
    for case in R.POOL_CASES:
        def margin(seed):
            x, Wp, _ = R.pool_case_inputs(case, seed)
            return float(R.maxpool(x, Wp)[2].min())
        pool_seeds.append(R.search_seed(margin))
    out["pool_seeds"] = np.array(pool_seeds, dtype=np.int64)
    cfg = dict(n_knn=R.ENC["n_knn"], target_latent_dim=R.ENC["latent"])
    for pooling in ("mean", "max"):
        for mode in ("train", "eval"):
            seed = next(s for s in range(2000) if encoder_ok(s, pooling, mode == "train"))
            out[f"{pooling}_{mode}_seed"] = np.array(seed, dtype=np.int64)
            P, x = R.encoder_params(seed, pooling), R.encoder_input(seed)
            g1, g2 = R.encoder_cotangents(seed)
            net = vn_encoder(dict(cfg, pooling=pooling)).double()
            net.load_state_dict(P, strict=True)
            net.train(mode == "train")
            with reference_run():
                gf, pf = net(x)
            assert gf.dtype == torch.float64 and pf.dtype == torch.float64
            out[f"{pooling}_{mode}_global"] = R.to_np(gf)
            out[f"{pooling}_{mode}_point_sub"] = R.to_np(pf[:, :, ::POINT_STRIDE])
            if mode == "train":
                ((gf * g1).sum() + (pf * g2).sum()).backward()
                for k, p in net.named_parameters():
                    if "pool" in k:
                        assert p.grad is None, k               # VNMaxPool's map_to_dir takes no gradient
                        continue
                    out[f"{pooling}_grad.{k}"] = R.to_np(grad_sub(p.grad))
                for k, v in net.state_dict().items():
                    if "running" in k:
                        out[f"{pooling}_stat.{k}"] = R.to_np(v)
            ret = vn_retrieval(dict(cfg, pooling=pooling)).double()
            ret.load_state_dict({k: v for k, v in P.items() if not k.startswith("per_point_f")}, strict=True)
            ret.train(mode == "train")
            with reference_run():
                out[f"ret_{pooling}_{mode}_global"] = R.to_np(ret(x))
    path = os.path.join(HERE, "vn.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; seeds:", {k: out[k].tolist() for k in out if "seed" in k})


if __name__ == "__main__":
    main(sys.argv[1])
