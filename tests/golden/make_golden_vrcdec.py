"""Writes tests/golden/vrcdec.npz: the float64, eval-mode outputs and gradients of the reference's
EF_expansion (Density_aware_Chamfer_Distance/utils/model_utils.py:137-166), Folding and MSAP_SKN_decoder
(models/vrcnet.py:54-86, 293-403). Run on a machine that has the reference tree (never on the GPU box):

    python tests/golden/make_golden_vrcdec.py <reference root>

Works as make_golden_vrcnet.py does, and reuses its `lift`, its float64 `pn2` stand-in and its no_cuda /
CpuTorch shims: the classes, get_graph_feature and what they call are lifted from the reference's source with
`ast`; the decoder's encoder gets the fixture's pts_num after construction (the reference's constructor has no
such argument). Only data goes into the npz: the seeds, the smallest decision ratios, the outputs, the decision
indices (feature-space kNN of the EF units, the decoder's FPS and score ranking, the encoder's FPS), the
state_dict key lists and shapes, and at most GRAD_CAP strided elements of every gradient under fixed
cotangents. Weights and inputs are regenerated from the seed by tests/vrcdec_ref.py (asserted here).

Each fixture's seed is the first one, searching upward from 0, that satisfies the rule in tests/vrcdec_ref.py's
docstring; the float32 restatement must then make the same decisions (asserted), and the smallest ratio is
printed.
"""
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
sys.path.insert(0, HERE)
import vrc_ref as R  # noqa: E402
import vrcdec_ref as D  # noqa: E402
from make_golden_vrcnet import CpuTorch, MAX_BYTES, Pn2, lift, no_cuda  # noqa: E402

SEED_LIMIT = 256


class Pn2Log(Pn2):
    """Pn2 that also logs the indices of every gather_operation."""

    def gather_operation(self, features, idx):
        self.log.setdefault("gather", []).append(idx.long())
        return Pn2.gather_operation(features, idx)


def qualify(name, seed):
    """-> the smallest gap / tolerance over the value-dependent decisions of the fixture, or None when a geometric
    margin of its encoder is below GEO_MARGIN or a ratio is below MARGIN_MULT."""
    r64 = D.run_fixture(name, torch.float64, seed=seed, grads=False)
    enc = r64["dec"].enc
    if any(enc.margin[k] < R.GEO_MARGIN for k in D.geo_names(enc)):
        return None
    r32 = D.run_fixture(name, torch.float32, seed=seed, grads=False)
    ratios = D.decision_ratios(r64, r32)
    if min(ratios.values()) < D.MARGIN_MULT:
        return None
    for k, v in r64["dec"].idx.items():                           # float32 makes the same decisions
        if not k.endswith(".slot"):
            assert torch.equal(v, r32["dec"].idx[k]), (seed, name, k)
    for k, v in enc.idx.items():
        if not k.startswith(("slot", "win")):
            assert torch.equal(v, r32["dec"].enc.idx[k]), (seed, name, k)
    return min(ratios.values())


def search(name):
    for seed in range(SEED_LIMIT):
        ratio = qualify(name, seed)
        if ratio is not None:
            print(name, "seed", seed, "smallest ratio", repr(ratio))
            return seed, ratio
    raise AssertionError(f"{name}: no seed below {SEED_LIMIT} qualifies")


def grads_of(outs, cots, mod, leaves):
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    g = {k: R.grad_sub(p.grad).numpy() for k, p in mod.named_parameters() if p.grad is not None}
    none = [k for k, p in mod.named_parameters() if p.grad is None]
    for i, t in enumerate(leaves):
        g[f"in{i}"] = R.grad_sub(t.grad).numpy()
    return g, none


def main(ref):
    seeds = {"fold": 0}                                           # Folding makes no value-dependent decision
    out = {}
    for name in ("ef", "dec_fold", "dec_ef"):
        seeds[name], ratio = search(name)
        out[f"ratio/{name}"] = np.array(ratio)
        out[f"ratio/{name}"] = np.array(D.GOLDEN_RATIOS[name])     # as recorded; float32 on another CPU moves it by a percent or so
        assert abs(ratio - D.GOLDEN_RATIOS[name]) <= 0.1 * ratio, f"{name}: tests/vrcdec_ref.py says {D.GOLDEN_RATIOS[name]}"
    assert seeds == D.GOLDEN_SEEDS, f"the first qualifying seeds are {seeds}; tests/vrcdec_ref.py says {D.GOLDEN_SEEDS}"
    for name, sd in seeds.items():
        out[f"seed/{name}"] = np.array(sd)
    pn2 = Pn2Log()
    ns = {"torch": CpuTorch(), "nn": nn, "F": F, "np": np, "pn2": pn2, "math": math}
    lift(ref, "Density_aware_Chamfer_Distance/utils/model_utils.py",
         ["knn", "knn_point", "get_edge_features", "edge_preserve_sampling", "three_nn_upsampling", "get_graph_feature",
          "EF_expansion"], ns)
    lift(ref, "Density_aware_Chamfer_Distance/models/vrcnet.py",
         ["SA_module", "SK_SA_module", "SKN_Res_unit", "SA_SKN_Res_encoder", "Folding", "MSAP_SKN_decoder"], ns)
    knn_ref, knn_log = ns["knn"], []

    def knn_logged(x, k):
        idx = knn_ref(x, k)
        knn_log.append((x.shape[1], idx))
        return idx
    ns["knn"] = knn_logged
    def same(mod, P, scaled=()):
        sd = mod.state_dict()
        assert list(sd) == list(P)
        assert all(torch.equal(sd[k], P[k]) for k in sd if not k.startswith(scaled))

    def keys(name, mod):
        sd = mod.state_dict()
        out[f"{name}/keys"] = np.array(list(sd))
        out[f"{name}/shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])

    with no_cuda():
        E = D.EF
        Pr, (x,), cots = D.fixture("ef")
        torch.manual_seed(seeds["ef"])
        mod = ns["EF_expansion"](E["C"], E["O"], E["r"], E["k"])
        same(mod, Pr)
        keys("ef", mod)
        mod = mod.double().eval()
        xg = x.double().requires_grad_(True)
        del knn_log[:]
        y = mod(xg)
        out["ef/out0"] = y.detach().numpy()
        out["ef/knn"] = knn_log[0][1].numpy().astype(np.int16)
        g, none = grads_of([y], cots, mod, [xg])
        assert not none
        for k, v in g.items():
            out[f"ef/g/{k}"] = v

        Fo = D.FOLD
        Pr, (x, gf), cots = D.fixture("fold")
        torch.manual_seed(seeds["fold"])
        mod = ns["Folding"](Fo["C"], Fo["output_size"], Fo["step_ratio"], Fo["G"])
        same(mod, Pr)
        keys("fold", mod)
        mod = mod.double().eval()
        xg, gg = x.double().requires_grad_(True), gf.double().requires_grad_(True)
        y = mod(xg, gg)
        out["fold/out0"] = y.detach().numpy()
        g, none = grads_of([y], cots, mod, [xg, gg])
        assert not none
        for k, v in g.items():
            out[f"fold/g/{k}"] = v
        for r in (1, 2, 3, 4, 6):                                 # the reference's grids, as data
            out[f"grid/{r}"] = ns["Folding"](4, 4, r, 4).grid.numpy()

        for name, cfg in D.DECS.items():
            Pr, (gf, pin), cots = D.fixture(name)
            torch.manual_seed(seeds[name])
            mod = ns["MSAP_SKN_decoder"](cfg["num_coarse_raw"], cfg["num_fps"], cfg["num_coarse"], cfg["num_fine"], cfg["layers"],
                                         cfg["knn_list"], cfg["pk"], cfg["points_label"], cfg["local_folding"], cfg["over_scale"])
            mod.encoder.pts_num = cfg["pts_num"]
            same(mod, Pr, scaled=("fc3.", "conv_s3."))
            keys(name, mod)
            mod.load_state_dict(Pr, strict=True)                  # the fixture's fc3 / conv_s3 scaling
            mod = mod.double().eval()
            gg, pg = gf.double().requires_grad_(True), pin.double().requires_grad_(True)
            pn2.log = {"fps": [], "three_nn": [], "gather": []}
            del knn_log[:]
            outs = mod(gg, pg)
            for i, o in enumerate(outs):
                out[f"{name}/out{i}"] = o.detach().numpy()
            g, none = grads_of(outs, cots, mod, [gg, pg])
            assert sorted(none) == sorted(f"conv_s{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")), none
            for k, v in g.items():
                out[f"{name}/g/{k}"] = v
            fps = pn2.log["fps"]
            assert len(fps) == 4                                  # the encoder's three, then the decoder's own
            for i, t in enumerate(fps[:3]):
                out[f"{name}/enc_fps{i + 1}"] = t.numpy().astype(np.int16)
            out[f"{name}/fps"] = fps[3].numpy().astype(np.int16)
            feat_knn = [idx for dims, idx in knn_log if dims != 3]
            tags = (["exp1"] if D.up_scale(cfg) >= 2 else []) + ([] if cfg["local_folding"] else ["exp2"])
            assert len(feat_knn) == len(tags)
            for tag, idx in zip(tags, feat_knn):
                out[f"{name}/knn/{tag}"] = idx.numpy().astype(np.int16)
            out[f"{name}/topk"] = pn2.log["gather"][-1].numpy().astype(np.int16)     # the decoder's last gather: idx_scores
    path = os.path.join(HERE, "vrcdec.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("wrote vrcdec.npz", size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
