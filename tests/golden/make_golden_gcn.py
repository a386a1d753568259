"""Writes tests/golden/gcn.npz: inputs, seeds, module weights and the float64 outputs and gradients
of the reference's network/P_3DGC.py (Conv_surface, Conv_layer, Pool_layer, the index helpers) and
network/gc3d_encoder.py (GCN3D_ENCODER). Run on a machine that has the reference tree (never on the
GPU box):

    python tests/golden/make_golden_gcn.py <reference root>

The reference modules are imported from <reference root> and run in float64; while they run,
torch.Tensor.float is the identity (get_neighbor_direction_norm ends in .float(), which would
otherwise drop the float64 run to float32) and torch.randperm is recorded. Only data goes into the
npz. The encoder's weights are not stored: tests/gcn_ref.py::encoder_params regenerates them from
the recorded seed. Of the encoder's per-point features every FEAT_STRIDE-th point is stored (the
whole tensor would not fit the 512 KB limit); tests/test_gcn_ref.py pins gcn_ref.encoder to them,
and the GPU test compares the whole tensor with gcn_ref.encoder in float64.

Seeds are searched until the conditions hold that make a GPU comparison meaningful, for the
reference alone (tests/test_gcn_ref.py asserts them again):
  kernel cases: theta == 0 occurs; every product is exact in fp32; every maximum that is not an exact
    0 leads its runner-up by more than 1e-5 * max|product| or ties with it exactly (with exact
    products a tie is the same tie in fp32 and falls to the stated lowest-slot rule; a cloud of 130
    vertices has 2 * 10^5 maxima, too many for continuous values to keep all of them that far apart);
  clouds: every K-NN row's sorted float64 distances through rank n + 2 differ by more than 1e-6, and
    every nearest-vertex choice leads the second by more than 1e-6;
  the Conv_layer gradient case: no theta within 2e-6 of 0, no winner within 1e-5 * max of its runner-up.
"""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gcn_ref as R  # noqa: E402

FEAT_STRIDE = 16
MOD = dict(B=2, V=64, n=4, S=3, cin=4, cout=8)


class reference_run:
    """float64 stays float64, and the randperm draws are recorded."""

    def __init__(self):
        self.samples = []

    def __enter__(self):
        self.saved = (torch.Tensor.float, torch.randperm)
        torch.Tensor.float = lambda t, *a, **k: t

        def randperm(*a, **k):
            p = self.saved[1](*a, **k)
            self.samples.append(p.clone())
            return p
        torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        torch.Tensor.float, torch.randperm = self.saved


def main(root):
    sys.path.insert(0, root)
    import network.P_3DGC as ref
    import network.gc3d_encoder as ref_enc
    out = {}

    # ---- kernel-level seeds ----
    seeds = np.zeros((len(R.KERNEL_CASES), 2), np.int64)
    for ci, case in enumerate(R.KERNEL_CASES):
        for layer in (0, 1):
            for seed in range(1000):
                if R.kernel_case_ok(case, seed, bool(layer)):
                    break
            else:
                raise SystemExit(f"no seed for kernel case {case} layer {layer}")
            seeds[ci, layer] = seed
    out["kern_seeds"] = seeds

    # ---- modules at 2 x 64 vertices ----
    m = MOD
    for seed in range(1000):
        rng = np.random.default_rng(1000 + seed)
        verts = torch.from_numpy(rng.random((m["B"], m["V"], 3)))
        if not R.cloud_ok(verts, m["n"]):
            continue
        W = {"surf.directions": rng.uniform(-0.3, 0.3, (3, m["S"] * m["cout"])),
             "layer.weights": rng.uniform(-0.3, 0.3, (m["cin"], (m["S"] + 1) * m["cout"])),
             "layer.bias": rng.uniform(-0.3, 0.3, ((m["S"] + 1) * m["cout"],)),
             "layer.directions": rng.uniform(-0.3, 0.3, (3, m["S"] * m["cout"]))}
        fmap = rng.standard_normal((m["B"], m["V"], m["cin"]))
        pmap = rng.standard_normal((m["B"], m["V"], m["cout"]))
        g = rng.standard_normal((m["B"], m["V"], m["cout"]))
        gp = rng.standard_normal((m["B"], m["V"] // 4, m["cout"]))
        idx = R.get_neighbor_index(verts, m["n"])
        if R.layer_case_ok(torch.from_numpy(W["layer.weights"]), torch.from_numpy(W["layer.bias"]),
                           torch.from_numpy(W["layer.directions"]), m["S"], idx, verts, torch.from_numpy(fmap)):
            break
    else:
        raise SystemExit("no seed for the module case")
    out["mod_seed"] = np.int64(1000 + seed)
    out["mod_vertices"], out["mod_fmap"], out["mod_pmap"], out["mod_g"], out["mod_gp"] = verts.numpy(), fmap, pmap, g, gp
    for k, v in W.items():
        out["mod_" + k] = v
    t = torch.from_numpy
    with reference_run() as rr:
        ridx = ref.get_neighbor_index(verts, m["n"])
        assert (ridx == idx).all(), "module cloud: the reference's neighbours differ from the restatement's"
        out["mod_idx"] = ridx.numpy().astype(np.int32)
        surf = ref.Conv_surface(m["cout"], m["S"]).double()
        surf.directions.data.copy_(t(W["surf.directions"]))
        y = surf(ridx, verts)
        y.backward(t(g))
        out["mod_surf_out"], out["mod_surf_gdir"] = y.detach().numpy(), surf.directions.grad.numpy()
        lay = ref.Conv_layer(m["cin"], m["cout"], m["S"]).double()
        for k in ("weights", "bias", "directions"):
            getattr(lay, k).data.copy_(t(W["layer." + k]))
        fm = t(fmap).clone().requires_grad_(True)
        y = lay(ridx, verts, fm)
        y.backward(t(g))
        out["mod_layer_out"] = y.detach().numpy()
        out["mod_layer_gw"], out["mod_layer_gb"] = lay.weights.grad.numpy(), lay.bias.grad.numpy()
        out["mod_layer_gdir"], out["mod_layer_gx"] = lay.directions.grad.numpy(), fm.grad.numpy()
        torch.manual_seed(77)
        out["mod_pool_seed"] = np.int64(77)
        pm = t(pmap).clone().requires_grad_(True)
        vp, fp = ref.Pool_layer(4, 4)(verts, pm)
        fp.backward(t(gp))
        out["mod_pool_sample"] = rr.samples[-1][:m["V"] // 4].numpy().astype(np.int32)
        out["mod_pool_v"], out["mod_pool_out"], out["mod_pool_gx"] = vp.numpy(), fp.detach().numpy(), pm.grad.numpy()
        out["mod_nearest"] = ref.get_nearest_index(verts, vp).numpy().astype(np.int32)

    # ---- encoder at 2 x 128 and 2 x 256 points ----
    for V in (128, 256):
        for seed in range(1000):
            pseed, rseed = 5000 + V + seed, 9000 + seed
            verts = torch.from_numpy(np.random.default_rng(pseed).random((2, V, 3)))
            if R.encoder_clouds_ok(verts, rseed):
                break
        else:
            raise SystemExit(f"no seed for the encoder cloud V={V}")
        out[f"enc{V}_vertices"], out[f"enc{V}_seeds"] = verts.numpy(), np.array([pseed, rseed, 31 + V], np.int64)
        P = R.encoder_params(31 + V)
        for mode in ("train", "eval"):
            net = ref_enc.GCN3D_ENCODER().double()
            net.load_state_dict(P, strict=True)
            net.train(mode == "train")
            torch.manual_seed(rseed)
            with reference_run() as rr, torch.no_grad():
                fg, feat = net(verts)
            sd = net.state_dict()
            out[f"enc{V}_{mode}_fglobal"] = fg.numpy()
            out[f"enc{V}_{mode}_feat_sub"] = feat[:, :, ::FEAT_STRIDE].numpy()
            if mode == "train":
                out[f"enc{V}_samples0"] = rr.samples[0][:V // 4].numpy().astype(np.int32)
                out[f"enc{V}_samples1"] = rr.samples[1][:V // 16].numpy().astype(np.int32)
                for k in sorted(sd):
                    if "running_" in k:
                        out[f"enc{V}_train_{k}"] = sd[k].numpy()
    path = os.path.join(HERE, "gcn.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, f"gcn.npz is {size} bytes"
    print("wrote", path, size, "bytes; kernel seeds", seeds.tolist(), "module seed", int(out["mod_seed"]))


if __name__ == "__main__":
    main(sys.argv[1])
