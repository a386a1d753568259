"""Writes tests/golden/group.npz: inputs and the outputs of the reference's
network/pointnet/pointnet2_utils.py (farthest_point_sample, query_ball_point, sample_and_group and
one PointNetSetAbstraction layer in float64) on them. Run on a machine that has the reference tree
(never on the GPU box):

    python tests/golden/make_golden_group.py <reference root>

The reference file is loaded by path with importlib; torch.randint is replaced while it runs, so
that farthest_point_sample starts at the fixture's `start`. Only data goes into the npz.

Clouds have coordinates k/g, k integer in [-g, g], g in {8, 16, 64}, and the radii are 0.125, 0.25
and 0.5: every product and sum of the reference's |a|^2 + |b|^2 - 2ab and of the plain
((dx*dx) + (dy*dy)) + (dz*dz) is then exact in fp32, so the two agree bit for bit while the clouds
are full of distance ties and of points exactly on a ball's surface. The script asserts that the
reference equals tests/group_ref.py on every row, that the ball-query set holds padded rows, full
rows and exact-boundary hits, and that the layer's ReLU / max-pool decisions are further from
flipping than twice the forward tolerance of tests/test_group_gpu.py.
"""
import importlib.util
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import group_ref as R  # noqa: E402

SA = dict(npoint=32, radius=0.25, nsample=16, in_channel=3 + 5, mlp=[16, 32], group_all=False)
BALLS = [(0.25, 16), (0.5, 32), (0.125, 8)]


def load_reference(root):
    path = os.path.join(root, "network", "pointnet", "pointnet2_utils.py")
    spec = importlib.util.spec_from_file_location("_reference_pointnet2_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class fixed_start:
    """torch.randint -> the fixture's start indices, while the reference's sampling runs."""

    def __init__(self, start):
        self.start = torch.as_tensor(np.asarray(start), dtype=torch.long)

    def __enter__(self):
        self.saved = torch.randint
        torch.randint = lambda *a, **k: self.start.clone()

    def __exit__(self, *exc):
        torch.randint = self.saved


def grid_cloud(rng, B, N, g):
    return (rng.integers(-g, g + 1, size=(B, N, 3)).astype(np.float32) / np.float32(g)).astype(np.float32)


def main(root):
    ref = load_reference(root)
    rng = np.random.default_rng(20240611)
    out = {}

    # ---- farthest-point sampling ----
    fps_cases = {"a": (grid_cloud(rng, 3, 64, 8), 16), "b": (grid_cloud(rng, 2, 1000, 64), 128),
                 "c": (grid_cloud(rng, 2, 2048, 16), 512)}
    dup = grid_cloud(rng, 2, 300, 8)
    dup[:, 150:] = dup[:, :150][:, rng.permutation(150)]          # every point twice
    fps_cases["d"] = (dup, 300)
    for name, (xyz, npoint) in fps_cases.items():
        B, N, _ = xyz.shape
        start = rng.integers(0, N, size=B).astype(np.int32)
        with fixed_start(start):
            got = ref.farthest_point_sample(torch.from_numpy(xyz), npoint).numpy()
        assert (got == R.fps(xyz, start, npoint)).all(), f"fps {name}: the reference differs from the restatement"
        out[f"fps_{name}_xyz"], out[f"fps_{name}_start"], out[f"fps_{name}_idx"] = xyz, start, got.astype(np.int32)

    # ---- ball query on the 2048 cloud, the queries its 512 samples ----
    xyz = fps_cases["c"][0]
    fi = out["fps_c_idx"]
    new_xyz = xyz[np.arange(2)[:, None], fi]
    out["ball_new_xyz"] = new_xyz
    padded = full = boundary = 0
    for r, ns in BALLS:
        got = ref.query_ball_point(r, ns, torch.from_numpy(xyz), torch.from_numpy(new_xyz)).numpy()
        assert (got == R.ball_query(xyz, new_xyz, R.radius2(r), ns)).all(), f"ball ({r}, {ns}): reference != restatement"
        out[f"ball_{r}_{ns}"] = got.astype(np.int32)
        d = R.sqd(xyz[:, None, :, :], new_xyz[:, :, None, :])
        hits = (~(d > R.radius2(r))).sum(-1)
        padded += int((hits < ns).sum())
        full += int((hits >= ns).sum())
        first = np.take_along_axis(d, got.astype(np.int64), axis=-1)      # distances of the listed indices
        boundary += int((first == R.radius2(r)).sum())
    assert padded > 0 and full > 0 and boundary > 0, (padded, full, boundary)
    print(f"ball query rows: {padded} padded, {full} full, {boundary} listed points exactly on the surface")

    # ---- sample_and_group and one set-abstraction layer ----
    B, N, D = 2, 256, 5
    xyz = grid_cloud(rng, B, N, 8)
    pts = rng.standard_normal((B, N, D)).astype(np.float32)
    start = rng.integers(0, N, size=B).astype(np.int32)
    with fixed_start(start):
        nx, npts, gxyz, fidx = ref.sample_and_group(SA["npoint"], SA["radius"], SA["nsample"], torch.from_numpy(xyz),
                                                    torch.from_numpy(pts), returnfps=True)
    idx = R.ball_query(xyz, nx.numpy(), R.radius2(SA["radius"]), SA["nsample"])
    assert (fidx.numpy() == R.fps(xyz, start, SA["npoint"])).all()
    assert (npts.numpy().reshape(-1, 3 + D) == R.group_fwd(xyz, nx.numpy(), pts, idx)).all()
    out.update(sa_xyz=xyz, sa_points=pts, sa_start=start, sg_new_xyz=nx.numpy(), sg_new_points=npts.numpy(),
               sg_grouped_xyz=gxyz.numpy(), sg_fps_idx=fidx.numpy().astype(np.int32), sg_idx=idx)

    x_bcn = np.ascontiguousarray(xyz.transpose(0, 2, 1))
    p_bdn = np.ascontiguousarray(pts.transpose(0, 2, 1))
    g_out = rng.standard_normal((B, SA["mlp"][-1], SA["npoint"])).astype(np.float32)
    g_xyz = rng.standard_normal((B, 3, SA["npoint"])).astype(np.float32)
    for seed in range(5000):
        torch.manual_seed(seed)
        layer = ref.PointNetSetAbstraction(**SA)
        with torch.no_grad():
            for bn in layer.mlp_bns:
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.normal_(0.0, 0.2)
                bn.running_mean.normal_(0.0, 0.5)
                bn.running_var.uniform_(0.5, 2.0)
        sd = {k: v.numpy().copy() for k, v in layer.state_dict().items()}
        r64 = R.sa_layer(sd, x_bcn, p_bdn, start, SA["npoint"], SA["radius"], SA["nsample"], False, torch.float64,
                         g_out, g_xyz)
        r32 = R.sa_layer(sd, x_bcn, p_bdn, start, SA["npoint"], SA["radius"], SA["nsample"], False, torch.float32,
                         g_out, g_xyz)
        tol = 3 * np.abs(r32["out"] - r64["out"]).max() + 1e-5 * np.abs(r64["out"]).max()
        relu_m, gap = R.decision_margin(r64["pre"])
        if relu_m > 2 * tol and gap > 2 * tol:
            print(f"weight seed {seed}: forward tolerance {tol:.3e}, smallest |pre-activation| {relu_m:.3e}, "
                  f"smallest pool gap {gap:.3e}")
            break
    else:
        raise SystemExit("no weight seed keeps the decisions clear of the tolerance")

    # the golden values: the reference's own layer, in float64
    layer = layer.double().train()
    x = torch.tensor(x_bcn, dtype=torch.float64, requires_grad=True)
    p = torch.tensor(p_bdn, dtype=torch.float64, requires_grad=True)
    torch.set_default_dtype(torch.float64)            # the tensors the reference creates itself (torch.ones)
    with fixed_start(start):
        new_xyz, new_points = layer(x, p)
    torch.set_default_dtype(torch.float32)
    loss = (new_points * torch.tensor(g_out, dtype=torch.float64)).sum() + \
        (new_xyz * torch.tensor(g_xyz, dtype=torch.float64)).sum()
    loss.backward()
    for k in ("out", "new_xyz", "gxyz", "gpoints"):
        got = {"out": new_points, "new_xyz": new_xyz, "gxyz": x.grad, "gpoints": p.grad}[k].detach().numpy()
        assert np.abs(got - r64[k]).max() <= 1e-12 * max(1.0, np.abs(got).max()), f"layer {k}: reference != restatement"
        out[f"sa_ref_{k}"] = got
    for k, v in layer.named_parameters():
        assert np.abs(v.grad.numpy() - r64["grads"][k]).max() <= 1e-11 * max(1.0, np.abs(v.grad.numpy()).max()), k
        out[f"sa_grad_{k}"] = v.grad.numpy()
    for k, v in layer.state_dict().items():
        if "running" in k:
            assert np.abs(v.numpy() - r64["running"][k]).max() <= 1e-12, k
            out[f"sa_after_{k}"] = v.numpy()
    for k, v in sd.items():
        out[f"sa_sd_{k}"] = v
    out["sa_g_out"], out["sa_g_xyz"] = g_out, g_xyz
    path = os.path.join(HERE, "group.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
