"""Writes tests/golden/vrcnet.npz: the float64, eval-mode outputs and gradients of the reference's
SA_module, SK_SA_module, SKN_Res_unit, SA_SKN_Res_encoder and Linear_ResBlock
(Density_aware_Chamfer_Distance/models/vrcnet.py:15-290). Run on a machine that has the reference
tree (never on the GPU box):

    python tests/golden/make_golden_vrcnet.py <reference root>

The five classes, and knn, knn_point, get_edge_features, edge_preserve_sampling and three_nn_upsampling
of utils/model_utils.py, are lifted from the reference's source with `ast`. Its pointnet2 extension is
CUDA-only; the `pn2` handed to the lifted code is a float64 torch stand-in written from the contracts
of the extension's kernels: farthest-point sampling from index 0 on the direct squared distance, three_nn
by an ascending scan with a strict `<` returning the square root, gather, grouping and
three_interpolate. While the lifted code runs, Tensor.cuda returns the tensor itself and
torch.device('cuda') resolves to the CPU.

Only data goes into the npz: the seed, the outputs, the decision indices and at most GRAD_CAP strided
elements of every parameter and input gradient under fixed cotangents. Weights and inputs are not
stored: tests/vrc_ref.py regenerates them from the seed (asserted here). The seed is the first one,
searching upward from 0, for which every geometric decision of the encoder fixture (the rank gaps among
the first k + 1 neighbours at all four levels, the FPS winner against the runner-up, the pk ranks and
the first four ranks of each three-NN) is at least GEO_MARGIN in squared distance from a flip.
"""
import ast
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
import vrc_ref as R  # noqa: E402

MAX_BYTES = 512 * 1024


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


class CpuTorch:
    """torch, with device('cuda') resolving to the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*a, **k):
        return torch.device("cpu")


class Pn2:
    """float64 stand-ins for the pointnet2 extension. `log` collects the decisions."""

    def __init__(self):
        self.log = {"fps": [], "three_nn": []}

    def furthest_point_sample(self, xyz, npoint):
        idx, _ = R.fps_pick(xyz.detach(), npoint)
        self.log["fps"].append(idx)
        return idx.int()

    @staticmethod
    def gather_operation(features, idx):
        return torch.gather(features, 2, idx.long().unsqueeze(1).expand(-1, features.shape[1], -1))

    @staticmethod
    def grouping_operation(features, idx):
        B, C, N = features.shape
        flat = idx.long().reshape(B, 1, -1).expand(-1, C, -1)
        return torch.gather(features, 2, flat).view(B, C, *idx.shape[1:])

    def three_nn(self, unknown, known):
        B, N, _ = unknown.shape
        S = known.shape[1]
        d = R._d2(unknown.detach(), known.detach())           # the extension's three_nn carries no gradient
        best = torch.full((B, N, 3), 1e40, dtype=d.dtype)
        bi = torch.zeros(B, N, 3, dtype=torch.long)
        for s in range(S):                                   # ascending scan, strict <
            ds = d[:, :, s]
            c0, c1, c2 = ds < best[:, :, 0], ds < best[:, :, 1], ds < best[:, :, 2]
            nb, ni = best.clone(), bi.clone()
            nb[:, :, 2] = torch.where(c1, best[:, :, 1], torch.where(c2, ds, best[:, :, 2]))
            ni[:, :, 2] = torch.where(c1, bi[:, :, 1], torch.where(c2, torch.full_like(bi[:, :, 2], s), bi[:, :, 2]))
            nb[:, :, 1] = torch.where(c0, best[:, :, 0], torch.where(c1, ds, best[:, :, 1]))
            ni[:, :, 1] = torch.where(c0, bi[:, :, 0], torch.where(c1, torch.full_like(bi[:, :, 1], s), bi[:, :, 1]))
            nb[:, :, 0] = torch.where(c0, ds, best[:, :, 0])
            ni[:, :, 0] = torch.where(c0, torch.full_like(bi[:, :, 0], s), bi[:, :, 0])
            best, bi = nb, ni
        self.log["three_nn"].append(bi)
        return torch.sqrt(best), bi.int()

    @staticmethod
    def three_interpolate(features, idx, weight):
        B, C, S = features.shape
        N = idx.shape[1]
        g = torch.gather(features, 2, idx.long().reshape(B, 1, N * 3).expand(-1, C, -1)).view(B, C, N, 3)
        return (g * weight.unsqueeze(1).to(features.dtype)).sum(3)


def geo_margin(seed):
    """The smallest margin of the encoder fixture's geometric decisions, on the float32 points in float64."""
    E = R.ENC
    pts = R.make_points(seed, E["B"], E["pts_num"][0]).double()
    worst = float("inf")
    levels = [pts]
    for lv in range(1, 4):
        idx, gap = R.fps_pick(levels[-1], E["pts_num"][lv])
        nxt = torch.gather(levels[-1], 1, idx.unsqueeze(-1).expand(-1, -1, 3))
        worst = min(worst, gap, R.knn_pick(nxt, levels[-1], E["pk"])[1])
        levels.append(nxt)
    for p in levels:
        worst = min(worst, R.knn_pick(p, p, max(E["k"]))[1])
    for lv in range(3):
        worst = min(worst, R.knn_pick(levels[lv], levels[lv + 1], 3)[1])
    return worst


def grads_of(out, cot, mod, leaf):
    (out * cot).sum().backward()
    g = {k: R.grad_sub(p.grad).numpy() for k, p in mod.named_parameters()}
    g["in0"] = R.grad_sub(leaf.grad).numpy()
    return g


def main(ref):
    seed = 0
    while geo_margin(seed) < R.GEO_MARGIN:
        seed += 1
    assert seed == R.GOLDEN_SEED, f"the first qualifying seed is {seed}; tests/vrc_ref.py says {R.GOLDEN_SEED}"
    print("seed", seed, "margin", geo_margin(seed))
    pn2 = Pn2()
    ns = {"torch": CpuTorch(), "nn": nn, "F": F, "np": np, "pn2": pn2}
    lift(ref, "Density_aware_Chamfer_Distance/utils/model_utils.py",
         ["knn", "knn_point", "get_edge_features", "edge_preserve_sampling", "three_nn_upsampling"], ns)
    lift(ref, "Density_aware_Chamfer_Distance/models/vrcnet.py",
         ["SA_module", "SK_SA_module", "SKN_Res_unit", "SA_SKN_Res_encoder", "Linear_ResBlock"], ns)
    out = {"seed": np.array(seed)}

    def same(mod, P):
        sd = mod.state_dict()
        assert list(sd) == list(P) and all(torch.equal(sd[k], P[k]) for k in sd)

    with no_cuda():
        # one SA_module, one SK_SA_module, one SKN_Res_unit on a 16-point cloud
        for name, S, cls, make in (("sa", R.SA, "SA_module", R.make_sa_params), ("sk", R.SK, "SK_SA_module", R.make_sk_params)):
            args = (S["in_planes"], S["rel"], S["mid"], S["out_planes"], S["share"], S["k"])
            torch.manual_seed(seed)
            mod = ns[cls](*args)
            same(mod, make(seed, *args))
            mod = mod.double().eval()
            pts = R.make_points(seed, S["B"], S["N"]).double()
            ks = S["k"] if isinstance(S["k"], list) else [S["k"]]
            idxs = [ns["knn"](pts.transpose(1, 2), k) for k in ks]
            for i, (k, idx) in enumerate(zip(ks, idxs)):
                assert torch.equal(idx, R.knn_pick(pts, pts, k)[0])
                out[f"{name}/idx{i}"] = idx.numpy().astype(np.int16)
            x = R.make_features(seed, S["B"], S["in_planes"], S["N"]).double().unsqueeze(2).requires_grad_(True)
            y, _ = mod([x, idxs if name == "sk" else idxs[0]])
            out[f"{name}/out"] = y.detach().numpy()
            for k, g in grads_of(y, R.cotangent(seed, tuple(y.shape)), mod, x).items():
                out[f"{name}/g/{k}"] = g
        # Linear_ResBlock on an input with negative entries; its ReLU is in place, so it gets a copy
        L = R.LRB
        torch.manual_seed(seed)
        mod = ns["Linear_ResBlock"](L["input_size"], L["output_size"])
        same(mod, R.make_lrb_params(seed, L["input_size"], L["output_size"]))
        mod = mod.double().eval()
        x = R.fixture("lrb", seed)[1].double().requires_grad_(True)
        assert bool((x < 0).any())
        y = mod(x.clone())
        out["lrb/out"] = y.detach().numpy()
        for k, g in grads_of(y, R.cotangent(seed, tuple(y.shape)), mod, x).items():
            out[f"lrb/g/{k}"] = g
        U = R.UNIT
        torch.manual_seed(seed)
        mod = ns["SKN_Res_unit"](U["input_size"], U["output_size"], U["k"], U["layers"])
        same(mod, R.make_unit_params(seed, U["input_size"], U["output_size"], U["k"], U["layers"]))
        mod = mod.double().eval()
        pts = R.make_points(seed, U["B"], U["N"]).double()
        idxs = [ns["knn"](pts.transpose(1, 2), k) for k in U["k"]]
        x = R.make_features(seed, U["B"], U["input_size"], U["N"]).double().unsqueeze(2).requires_grad_(True)
        y = mod(x, idxs)
        out["unit/out"] = y.detach().numpy()
        for k, g in grads_of(y, R.cotangent(seed, tuple(y.shape)), mod, x).items():
            out[f"unit/g/{k}"] = g
        # the encoder
        E = R.ENC
        torch.manual_seed(seed)
        enc = ns["SA_SKN_Res_encoder"](E["C_in"], E["k"], E["pk"], E["output_size"], E["layers"], E["pts_num"])
        same(enc, R.make_encoder_params(seed, E["C_in"], E["k"], E["output_size"], E["layers"]))
        enc = enc.double().eval()
        x = R.make_encoder_input(seed, E["B"], E["C_in"], E["pts_num"][0]).double().requires_grad_(True)
        pn2.log = {"fps": [], "three_nn": []}
        y = enc(x)
        out["enc/out"] = y.detach().numpy()
        for k, g in grads_of(y, R.cotangent(seed, tuple(y.shape)), enc, x).items():
            out[f"enc/g/{k}"] = g
        for i, t in enumerate(pn2.log["fps"]):
            out[f"enc/fps{i + 1}"] = t.numpy().astype(np.int16)
        for i, t in enumerate(pn2.log["three_nn"]):          # conv7 (level 2), conv8 (level 1), conv9 (level 0)
            out[f"enc/three_nn{2 - i}"] = t.numpy().astype(np.int16)
    path = os.path.join(HERE, "vrcnet.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("wrote vrcnet.npz", size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
