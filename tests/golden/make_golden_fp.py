"""Writes tests/golden/fp.npz: inputs and the outputs of the reference's network/pointnet/
pointnet2_utils.py (one PointNetFeaturePropagation layer twice and one PointNetSetAbstractionMsg
layer, in float64, training mode) on them, and the state_dict key names and shapes of the
reference's six pointnet2_* models. Run on a machine that has the reference tree (never on the GPU
box):

    python tests/golden/make_golden_fp.py <reference root>

The reference files are loaded by path with importlib (models.pointnet2_utils / pointnet2_utils are
aliased to the loaded pointnet2_utils so that the model files import); torch.randint is replaced
while the sampling runs, as in make_golden_group.py. Only data goes into the npz: arrays, and for
the models names and shapes, no weights.

FP case a: B = 2, N = 192 uniform in [-1,1]^3, the coarse cloud its farthest-point sample of S = 48
(so d = 0 for 48 points of every cloud), D1 = 6, D2 = 10, mlp [32, 16]. FP case b: B = 4, N = 64,
S = 1, no points1, D2 = 12, mlp [16] (every fine point of a cloud gets the same row, so a channel has
only B distinct values in its batch statistics: with B = 2 they normalise to +-1 whatever the weights,
the true parameter gradients vanish and every computed one is cancellation noise; four clouds keep
the layer well conditioned). MSG: the sa_* grid-cloud recipe of group.npz (B = 2, N = 256,
coordinates k/8, D = 5), npoint 32, radii [0.25, 0.5], nsample [8, 16], mlp [[16, 32], [16, 24]].

The script asserts (and tests/test_fp_ref.py repeats) that (i) the float64 restatement of
tests/fp_ref.py equals the reference to 1e-11 relative on every stored array, (ii) in FP case a every
query's relative gap (d4 - d3) / d4 is at least 1e-3 (the cloud seed is searched), so fp32 and
float64 pick the same three neighbours, (iii) no ReLU pre-activation and, for MSG, no max-pool
winner's gap lies within twice the forward tolerance of tests/test_fp_gpu.py (the weight seed is
searched).
"""
import importlib.util
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
import fp_ref as R  # noqa: E402
import group_ref as GR  # noqa: E402
from make_golden_group import fixed_start, grid_cloud, load_reference  # noqa: E402

FPA = dict(B=2, N=192, S=48, D1=6, D2=10, mlp=[32, 16])
FPB = dict(B=4, N=64, S=1, D2=12, mlp=[16])
MSG = dict(npoint=32, radius_list=[0.25, 0.5], nsample_list=[8, 16], in_channel=5, mlp_list=[[16, 32], [16, 24]])
MODELS = {"pointnet2_cls_ssg": (40, True), "pointnet2_cls_msg": (40, True), "pointnet2_part_seg_ssg": (50, True),
          "pointnet2_part_seg_msg": (50, True), "pointnet2_sem_seg": (13,), "pointnet2_sem_seg_msg": (13,)}
MIN_GAP = 1e-3


def randomise_bn(layer):
    with torch.no_grad():
        for m in layer.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.2)
                m.running_mean.normal_(0.0, 0.5)
                m.running_var.uniform_(0.5, 2.0)


def close(got, want, what, rel=1e-11):
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    assert err <= rel * max(1.0, np.abs(want).max()), f"{what}: the reference differs from the restatement by {err:.3e}"


def tol_fwd(r32, r64):
    return 3 * np.abs(r32["out"] - r64["out"]).max() + 1e-5 * np.abs(r64["out"]).max()


def fp_case(ref, out, tag, cfg, rng, xyz1, xyz2):
    """Search the weight seed, run the reference's layer in float64, check and store."""
    B, N, S = cfg["B"], cfg["N"], cfg["S"]
    D1, D2, mlp = cfg.get("D1", 0), cfg["D2"], cfg["mlp"]
    p1 = rng.standard_normal((B, N, D1)).astype(np.float32) if D1 else None
    p2 = rng.standard_normal((B, S, D2)).astype(np.float32)
    g_out = rng.standard_normal((B, mlp[-1], N)).astype(np.float32)
    bcn = lambda a: None if a is None else np.ascontiguousarray(a.transpose(0, 2, 1))
    args = (bcn(xyz1), bcn(xyz2), bcn(p1), bcn(p2))
    for seed in range(5000):
        torch.manual_seed(seed)
        layer = ref.PointNetFeaturePropagation(D1 + D2, mlp)
        randomise_bn(layer)
        sd = {k: v.numpy().copy() for k, v in layer.state_dict().items()}
        r64 = R.fp_layer(sd, *args, torch.float64, g_out)
        r32 = R.fp_layer(sd, *args, torch.float32, g_out)
        tol, m = tol_fwd(r32, r64), R.relu_margin(r64["pre"])
        if m > 2 * tol:
            print(f"fp {tag}: weight seed {seed}, forward tolerance {tol:.3e}, smallest |pre-activation| {m:.3e}")
            break
    else:
        raise SystemExit(f"fp {tag}: no weight seed keeps the decisions clear of the tolerance")
    layer = layer.double().train()
    t = [None if a is None else torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in args]
    torch.set_default_dtype(torch.float64)
    res = layer(*t)
    torch.set_default_dtype(torch.float32)
    (res * torch.tensor(g_out, dtype=torch.float64)).sum().backward()
    zero = lambda a: np.zeros(a.shape) if a.grad is None else a.grad.numpy()
    got = {"out": res.detach().numpy(), "gxyz1": zero(t[0]), "gxyz2": zero(t[1]), "gpoints2": t[3].grad.numpy()}
    if D1:
        got["gpoints1"] = t[2].grad.numpy()
    for k, v in got.items():
        close(r64[k], v, f"fp {tag} {k}")
        out[f"fp{tag}_ref_{k}"] = v
    for k, v in layer.named_parameters():
        close(r64["grads"][k], v.grad.numpy(), f"fp {tag} grad {k}")
        out[f"fp{tag}_grad_{k}"] = v.grad.numpy()
    for k, v in layer.state_dict().items():
        if "running" in k:
            close(r64["running"][k], v.numpy(), f"fp {tag} {k}")
            out[f"fp{tag}_after_{k}"] = v.numpy()
    for k, v in sd.items():
        out[f"fp{tag}_sd_{k}"] = v
    out[f"fp{tag}_xyz1"], out[f"fp{tag}_xyz2"], out[f"fp{tag}_points2"], out[f"fp{tag}_g_out"] = xyz1, xyz2, p2, g_out
    if D1:
        out[f"fp{tag}_points1"] = p1


def msg_case(ref, out, rng):
    B, N, D = 2, 256, MSG["in_channel"]
    xyz = grid_cloud(rng, B, N, 8)
    pts = rng.standard_normal((B, N, D)).astype(np.float32)
    start = rng.integers(0, N, size=B).astype(np.int32)
    x_bcn, p_bdn = (np.ascontiguousarray(a.transpose(0, 2, 1)) for a in (xyz, pts))
    C = sum(m[-1] for m in MSG["mlp_list"])
    g_out = rng.standard_normal((B, C, MSG["npoint"])).astype(np.float32)
    g_xyz = rng.standard_normal((B, 3, MSG["npoint"])).astype(np.float32)
    run = lambda sd, dt: R.msg_layer(sd, x_bcn, p_bdn, start, MSG["npoint"], MSG["radius_list"], MSG["nsample_list"], dt,
                                     g_out, g_xyz)
    for seed in range(5000):
        torch.manual_seed(seed)
        layer = ref.PointNetSetAbstractionMsg(**MSG)
        randomise_bn(layer)
        sd = {k: v.numpy().copy() for k, v in layer.state_dict().items()}
        r64, r32 = run(sd, torch.float64), run(sd, torch.float32)
        tol = tol_fwd(r32, r64)
        margins = [GR.decision_margin(p) for p in r64["pre"]]
        relu_m, gap = min(m[0] for m in margins), min(m[1] for m in margins)
        if relu_m > 2 * tol and gap > 2 * tol:
            print(f"msg: weight seed {seed}, forward tolerance {tol:.3e}, smallest |pre-activation| {relu_m:.3e}, "
                  f"smallest pool gap {gap:.3e}")
            break
    else:
        raise SystemExit("msg: no weight seed keeps the decisions clear of the tolerance")
    layer = layer.double().train()
    x = torch.tensor(x_bcn, dtype=torch.float64, requires_grad=True)
    p = torch.tensor(p_bdn, dtype=torch.float64, requires_grad=True)
    torch.set_default_dtype(torch.float64)
    with fixed_start(start):
        new_xyz, new_points = layer(x, p)
    torch.set_default_dtype(torch.float32)
    ((new_points * torch.tensor(g_out, dtype=torch.float64)).sum()
     + (new_xyz * torch.tensor(g_xyz, dtype=torch.float64)).sum()).backward()
    for k, v in (("out", new_points), ("new_xyz", new_xyz), ("gxyz", x.grad), ("gpoints", p.grad)):
        close(r64[k], v.detach().numpy(), f"msg {k}")
        out[f"msg_ref_{k}"] = v.detach().numpy()
    for k, v in layer.named_parameters():
        close(r64["grads"][k], v.grad.numpy(), f"msg grad {k}")
        out[f"msg_grad_{k}"] = v.grad.numpy()
    for k, v in layer.state_dict().items():
        if "running" in k:
            close(r64["running"][k], v.numpy(), f"msg {k}")
            out[f"msg_after_{k}"] = v.numpy()
    for k, v in sd.items():
        out[f"msg_sd_{k}"] = v
    out.update(msg_xyz=xyz, msg_points=pts, msg_start=start, msg_g_out=g_out, msg_g_xyz=g_xyz)


def model_keys(root, utils, out):
    """Names and shapes of the reference models' state dicts (data, no weights)."""
    for alias in ("pointnet2_utils", "models.pointnet2_utils"):
        sys.modules[alias] = utils
    sys.modules.setdefault("models", type(sys)("models"))
    for name, args in MODELS.items():
        path = os.path.join(root, "network", "pointnet", name + ".py")
        spec = importlib.util.spec_from_file_location("_reference_" + name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        sd = mod.get_model(*args).state_dict()
        out[f"model_{name}_keys"] = np.array(list(sd.keys()))
        shapes = np.full((len(sd), 4), -1, np.int64)
        for i, v in enumerate(sd.values()):
            shapes[i, :v.dim()] = list(v.shape)
        out[f"model_{name}_shapes"] = shapes


def main(root):
    ref = load_reference(root)
    out = {}
    # FP case a: the first cloud seed whose third neighbour is clear of the fourth everywhere
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        xyz1 = (rng.random((FPA["B"], FPA["N"], 3), dtype=np.float32) * 2 - 1).astype(np.float32)
        start = rng.integers(0, FPA["N"], size=FPA["B"]).astype(np.int32)
        xyz2, _ = R.fps_subset(xyz1, start, FPA["S"])
        gap = R.neighbour_gap(xyz1, xyz2)
        if gap >= MIN_GAP:
            print(f"fp a: cloud seed {seed}, smallest (d4 - d3) / d4 = {gap:.3e}")
            break
    else:
        raise SystemExit("fp a: no cloud seed keeps the third neighbour clear of the fourth")
    d, _ = R.three_nn(xyz1, xyz2)
    assert ((d[..., 0] == 0).sum(-1) == FPA["S"]).all()
    fp_case(ref, out, "a", FPA, rng, xyz1, xyz2)
    rng = np.random.default_rng(20240612)
    xyz1 = (rng.random((FPB["B"], FPB["N"], 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    fp_case(ref, out, "b", FPB, rng, xyz1, xyz1[:, 5:6].copy())
    msg_case(ref, out, rng)
    model_keys(root, ref, out)
    path = os.path.join(HERE, "fp.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(f"wrote {path}: {size} bytes, {len(out)} arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
