"""Plain restatements of the feature-propagation contracts of csrc/interp.hip (include/ured_hip.h):
the three nearest coarse points, the inverse-distance weights and the interpolation in numpy, fp32
in the stated operation order and float64, the three gradients as float64 sums with the inputs of
their error bounds, and one PointNetFeaturePropagation / PointNetSetAbstractionMsg layer in torch on
the CPU at a chosen precision. tests/golden/fp.npz pins the layers to the reference's
pointnet2_utils.py. TEST INFRASTRUCTURE ONLY."""
import numpy as np

import group_ref as GR
import knn_ref

F32 = np.float32
EPS32 = F32(1e-8)
EPS64 = np.float64(EPS32)          # the float64 weights use the kernel's fp32 constant
U = 2.0 ** -24


def three_nn(xyz1, xyz2, K=None):
    """xyz1 [B,N,3], xyz2 [B,S,3] -> (d2 [B,N,K] fp32, idx int32 [B,N,K]), K = min(3, S) unless given:
    ascending (distance, index) by knn's contract distance."""
    K = min(3, xyz2.shape[1]) if K is None else K
    return knn_ref.knn(np.asarray(xyz1, F32), np.asarray(xyz2, F32), K)


def fps_subset(xyz, start, S):
    """The coarse cloud of the tests: the farthest-point sample of the fine one (d = 0 for S points)."""
    fi = GR.fps(xyz, start, S)
    return xyz[np.arange(xyz.shape[0])[:, None], fi], fi


def weights32(d2):
    """r_k = 1.0f / (d_k + 1e-8f), R = (r_0 + r_1) + r_2, w_k = r_k / R, all fp32. -> (w, r)."""
    d2 = np.asarray(d2, F32)
    r = (F32(1.0) / (d2 + EPS32)).astype(F32)
    R = r[..., 0]
    for k in range(1, d2.shape[-1]):
        R = (R + r[..., k]).astype(F32)
    return (r / R[..., None]).astype(F32), r


def weights64(d2):
    d = np.asarray(d2, F32).astype(np.float64)
    r = 1.0 / (d + EPS64)
    return r / r.sum(-1, keepdims=True), r


def _gather(points2, idx):
    B = idx.shape[0]
    return points2[np.arange(B)[:, None, None], idx]            # [B,N,K,D2]


def interp_fwd32(points2, idx, d2, points1=None):
    """-> (out [B*N, D1 + D2] fp32 by the contract's order, w [B,N,K] fp32)."""
    w, _ = weights32(d2)
    f = _gather(np.asarray(points2, F32), idx)
    acc = (w[..., 0, None] * f[:, :, 0]).astype(F32)
    for k in range(1, idx.shape[-1]):
        acc = (acc + (w[..., k, None] * f[:, :, k]).astype(F32)).astype(F32)
    if points1 is not None:
        acc = np.concatenate([np.asarray(points1, F32), acc], -1)
    return acc.reshape(-1, acc.shape[-1]), w


def interp_fwd64(points2, idx, d2, points1=None):
    """-> (out float64 [B*N, D1 + D2], per element sum_k |w_k f_kc| (0 bound on the copied columns))."""
    w, _ = weights64(d2)
    f = _gather(np.asarray(points2, np.float64), idx)
    t = w[..., None] * f
    out, asum = t.sum(2), np.abs(t).sum(2)
    if points1 is not None:
        out = np.concatenate([np.asarray(points1, np.float64), out], -1)
        asum = np.concatenate([np.zeros(points1.shape), asum], -1)
    return out.reshape(-1, out.shape[-1]), asum.reshape(-1, asum.shape[-1])


def interp_bwd64(g, points2, idx, d2, D1):
    """g [B*N, D1 + D2] -> float64 gradients and the inputs of their bounds:
    gp2 [B,S,D2] with ap2 (sum of |terms|) and n2 [B,S] (terms per element); gd2 [B,N,K] with
    Te = r_k w_k sum_{j != k} w_j sum_c |g_c| (|f_kc| + |f_jc|); gp1 = g[:, :D1] (exact)."""
    B, N, K = idx.shape
    S, D2 = points2.shape[1], points2.shape[2]
    g64 = np.asarray(g, np.float64).reshape(B, N, -1)
    gi = g64[..., D1:]
    w, r = weights64(d2)
    f = _gather(np.asarray(points2, np.float64), idx)
    gp2, ap2, n2 = np.zeros((B, S, D2)), np.zeros((B, S, D2)), np.zeros((B, S), np.int64)
    for b in range(B):
        t = (w[b][..., None] * gi[b][:, None, :]).reshape(N * K, D2)
        j = idx[b].reshape(-1).astype(np.int64)
        np.add.at(gp2[b], j, t)
        np.add.at(ap2[b], j, np.abs(t))
        np.add.at(n2[b], j, 1)
    A = (gi[:, :, None, :] * f).sum(-1)                                         # [B,N,K]
    Aa = np.abs(gi)[:, :, None, :] * np.abs(f)                                  # |g_c| |f_kc|
    gd2, Te = np.zeros((B, N, K)), np.zeros((B, N, K))
    for k in range(K):
        for j in range(K):
            if j != k:
                gd2[..., k] += w[..., j] * (A[..., k] - A[..., j])
                Te[..., k] += w[..., j] * (Aa[:, :, k] + Aa[:, :, j]).sum(-1)
        gd2[..., k] *= -(r[..., k] * w[..., k])
        Te[..., k] *= r[..., k] * w[..., k]
    return dict(gp2=gp2, ap2=ap2, n2=n2, gd2=gd2, Te=Te, gp1=np.asarray(g).reshape(B, N, -1)[..., :D1])


def interp_bwd32(g, points2, idx, d2, D1):
    """The kernels' arithmetic in fp32: grad_points2 as a sequential sum from 0 over ascending (n,k)
    of the rounded products w * g; grad_d2 = -((r_k * w_k) * sum_{j != k} w_j * (A_k - A_j)), j
    ascending, A_k an fp32 dot product (numpy's summation order; the bound holds for any)."""
    B, N, K = idx.shape
    S, D2 = points2.shape[1], points2.shape[2]
    gi = np.asarray(g, F32).reshape(B, N, -1)[..., D1:]
    w, r = weights32(d2)
    p2 = np.asarray(points2, F32)
    gp2 = np.zeros((B, S, D2), F32)
    for b in range(B):
        for n in range(N):
            for k in range(K):
                j = idx[b, n, k]
                gp2[b, j] = (gp2[b, j] + (w[b, n, k] * gi[b, n]).astype(F32)).astype(F32)
    f = _gather(p2, idx)
    A = (gi[:, :, None, :] * f).astype(F32).sum(-1, dtype=F32)
    gd2 = np.zeros((B, N, K), F32)
    for k in range(K):
        s = None
        for j in range(K):
            if j != k:
                t = (w[..., j] * (A[..., k] - A[..., j]).astype(F32)).astype(F32)
                s = t if s is None else (s + t).astype(F32)
        if s is not None:
            gd2[..., k] = -((r[..., k] * w[..., k]).astype(F32) * s).astype(F32)
    return dict(gp2=gp2, gd2=gd2)


# ---------------- the layers in torch on the CPU ----------------

def _conv_bn_relu(T, sd, conv_key, bn_key, h, red, params, pres, running, eps, momentum):
    """One Conv(k=1) + BatchNorm (training) + ReLU on channels-last h; statistics over dims `red`."""
    import torch
    W = T(sd[f"{conv_key}.weight"]).requires_grad_(True)
    bias = T(sd[f"{conv_key}.bias"]).requires_grad_(True)
    gamma = T(sd[f"{bn_key}.weight"]).requires_grad_(True)
    beta = T(sd[f"{bn_key}.bias"]).requires_grad_(True)
    params.update({f"{conv_key}.weight": W, f"{conv_key}.bias": bias, f"{bn_key}.weight": gamma, f"{bn_key}.bias": beta})
    y = h @ W.view(W.shape[0], -1).t() + bias
    mean = y.mean(red)
    var = ((y - mean) ** 2).mean(red)
    pre = (y - mean) / torch.sqrt(var + eps) * gamma + beta
    pres.append(pre.detach().numpy())
    n = y.numel() // y.shape[-1]
    running[f"{bn_key}.running_mean"] = ((1 - momentum) * T(sd[f"{bn_key}.running_mean"]) + momentum * mean.detach()).numpy()
    running[f"{bn_key}.running_var"] = ((1 - momentum) * T(sd[f"{bn_key}.running_var"])
                                        + momentum * var.detach() * n / (n - 1)).numpy()
    return torch.relu(pre)


def fp_layer(sd, xyz1, xyz2, points1, points2, dtype, g_out, eps=1e-5, momentum=0.1):
    """One PointNetFeaturePropagation layer in training mode with plain torch ops at `dtype`; the
    neighbours are three_nn's (fp32 contract), distances and weights are formed at `dtype` from the
    coordinates (so both clouds get their gradient). sd: the layer's state dict (numpy); xyz1 [B,3,N],
    xyz2 [B,3,S], points1 [B,D1,N] | None, points2 [B,D2,S]; the loss is sum(out * g_out).
    -> dict: out [B,C,N], gxyz1, gxyz2, gpoints1 | None, gpoints2, grads, running, pre, idx."""
    import torch
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x1, x2, p2 = (T(a).requires_grad_(True) for a in (xyz1, xyz2, points2))
    p1 = None if points1 is None else T(points1).requires_grad_(True)
    B, _, N = x1.shape
    S = x2.shape[2]
    x1t, x2t, p2t = x1.permute(0, 2, 1), x2.permute(0, 2, 1), p2.permute(0, 2, 1)
    idx = None
    if S == 1:
        interp = p2t.repeat(1, N, 1)
    else:
        _, idx = three_nn(np.ascontiguousarray(np.asarray(xyz1, F32).transpose(0, 2, 1)),
                          np.ascontiguousarray(np.asarray(xyz2, F32).transpose(0, 2, 1)))
        il = torch.from_numpy(idx.astype(np.int64))
        bt = torch.arange(B)[:, None, None]
        d = ((x1t[:, :, None, :] - x2t[bt, il]) ** 2).sum(-1)
        r = 1.0 / (d + 1e-8)
        w = r / r.sum(-1, keepdim=True)
        interp = (p2t[bt, il] * w[..., None]).sum(2)
    h = interp if p1 is None else torch.cat([p1.permute(0, 2, 1), interp], -1)
    L = len([k for k in sd if k.startswith("mlp_convs.") and k.endswith(".weight")])
    params, pres, running = {}, [], {}
    for i in range(L):
        h = _conv_bn_relu(T, sd, f"mlp_convs.{i}", f"mlp_bns.{i}", h, (0, 1), params, pres, running, eps, momentum)
    out = h.permute(0, 2, 1)
    ins = [x1, x2, p2] + ([] if p1 is None else [p1])
    gr = torch.autograd.grad((out * T(g_out)).sum(), ins + list(params.values()), allow_unused=True)
    z = lambda t, like: np.zeros(like.shape) if t is None else t.numpy()
    return dict(out=out.detach().numpy(), gxyz1=z(gr[0], x1), gxyz2=z(gr[1], x2), gpoints2=gr[2].numpy(),
                gpoints1=None if p1 is None else gr[3].numpy(),
                grads={k: v.numpy() for k, v in zip(params, gr[len(ins):])}, running=running, pre=pres, idx=idx)


def msg_layer(sd, xyz, points, start, npoint, radius_list, nsample_list, dtype, g_out, g_xyz, eps=1e-5, momentum=0.1):
    """One PointNetSetAbstractionMsg layer in training mode with plain torch ops at `dtype` (sampling
    and ball queries by the fp32 contracts of group_ref); rows are cat([points, xyz - centre]), the
    reference's order. xyz [B,3,N], points [B,D,N] | None; loss sum(out * g_out) + sum(new_xyz * g_xyz).
    -> dict: new_xyz [B,3,S], out, gxyz, gpoints | None, grads, running, pre (per scale a list of
    [B,S,K,C_i]), fps_idx."""
    import torch
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x = T(xyz).requires_grad_(True)
    p = None if points is None else T(points).requires_grad_(True)
    B = x.shape[0]
    xt = x.permute(0, 2, 1)
    pt = None if p is None else p.permute(0, 2, 1)
    x32 = np.ascontiguousarray(np.asarray(xyz, F32).transpose(0, 2, 1))
    fi = GR.fps(x32, start, npoint)
    c32 = x32[np.arange(B)[:, None], fi]
    bt = torch.arange(B)
    new_xyz = xt[bt[:, None], torch.from_numpy(fi.astype(np.int64))]
    params, running, pres_all, outs = {}, {}, [], []
    for i, (radius, K) in enumerate(zip(radius_list, nsample_list)):
        il = torch.from_numpy(GR.ball_query(x32, c32, GR.radius2(radius), K).astype(np.int64))
        rows = xt[bt[:, None, None], il] - new_xyz[:, :, None, :]
        if pt is not None:
            rows = torch.cat([pt[bt[:, None, None], il], rows], -1)
        L = len([k for k in sd if k.startswith(f"conv_blocks.{i}.") and k.endswith(".weight")])
        pres, h = [], rows
        for j in range(L):
            h = _conv_bn_relu(T, sd, f"conv_blocks.{i}.{j}", f"bn_blocks.{i}.{j}", h, (0, 1, 2), params, pres, running,
                              eps, momentum)
        pres_all.append(pres)
        outs.append(h.max(2)[0])
    out = torch.cat(outs, -1).permute(0, 2, 1)
    nx = new_xyz.permute(0, 2, 1)
    loss = (out * T(g_out)).sum() + (nx * T(g_xyz)).sum()
    ins = [x] + ([] if p is None else [p])
    gr = torch.autograd.grad(loss, ins + list(params.values()))
    return dict(new_xyz=nx.detach().numpy(), out=out.detach().numpy(), gxyz=gr[0].numpy(),
                gpoints=None if p is None else gr[1].numpy(),
                grads={k: v.numpy() for k, v in zip(params, gr[len(ins):])}, running=running, pre=pres_all, fps_idx=fi)


def relu_margin(pres):
    """The smallest |BN output| over the layers: how far the nearest ReLU decision is from flipping."""
    return min(float(np.abs(p).min()) for p in pres)


def neighbour_gap(xyz1, xyz2):
    """min over the queries of (d4 - d3) / d4 (fp32 contract distances): how clearly the third
    neighbour is chosen. Needs S >= 4."""
    d, _ = three_nn(xyz1, xyz2, 4)
    d = d.astype(np.float64)
    return float(((d[..., 3] - d[..., 2]) / d[..., 3]).min())


# ---------------- the kernel-level cases and bounds (tests/test_fp_ref.py, tests/test_fp_gpu.py) ----------------

KERNEL_SHAPES = [(2, 256, 64, 37), (2, 200, 3, 5), (2, 130, 2, 64), (1, 300, 100, 131), (3, 65, 1, 4)]   # (B,N,S,D2)
D1S = (0, 6)
C_FWD, C_GP2, C_GD2 = 10.0, 8.0, 16.0    # forward 10 u; grad_points2 (n_e + 8) u; grad_d2 (D2 + 16) u


def kernel_case(B, N, S, D2, D1, coincident=False):
    """Inputs of one kernel-level case: a uniform fine cloud in [-1,1]^3, the coarse cloud its
    farthest-point sample (d = 0 for S of every N points; `coincident`: coarse point 1 moved onto
    coarse point 0), normal features and output gradient, and the restatement's neighbours."""
    rng = np.random.default_rng(1000 * N + 10 * S + D1 + (5 if coincident else 0))
    xyz1 = (rng.random((B, N, 3), dtype=F32) * 2 - 1).astype(F32)
    xyz2, _ = fps_subset(xyz1, rng.integers(0, N, size=B), S)
    xyz2 = xyz2.copy()
    if coincident:
        xyz2[:, 1] = xyz2[:, 0]
    c = dict(xyz1=xyz1, xyz2=xyz2, points2=rng.standard_normal((B, S, D2)).astype(F32),
             points1=rng.standard_normal((B, N, D1)).astype(F32) if D1 else None,
             g=rng.standard_normal((B * N, D1 + D2)).astype(F32), D1=D1)
    c["d2"], c["idx"] = three_nn(xyz1, xyz2)
    return c


def _worst(err, scale, what, const_name):
    """max err / (u * scale) over the elements with scale > 0; elements with scale 0 must be exact."""
    assert (err[scale == 0] == 0).all(), f"{what}: an element whose terms are all zero is not exact"
    ratio = float((err[scale > 0] / (U * scale[scale > 0])).max()) if (scale > 0).any() else 0.0
    print(f"{what}: max err {err.max():.3e}, needs {const_name} >= {ratio:.3f}")
    return ratio


def check_fwd(got, c):
    """|err| <= 10 u sum_k |w_k f_kc| on the interpolated columns; the copied columns exact."""
    ref, asum = interp_fwd64(c["points2"], c["idx"], c["d2"], c["points1"])
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    if c["D1"]:
        assert (got[:, :c["D1"]] == ref[:, :c["D1"]]).all(), "forward: the points1 columns are not a copy"
    err = np.abs(got - ref)[:, c["D1"]:]
    ratio = _worst(err, asum[:, c["D1"]:], "forward", "C")
    assert ratio <= C_FWD, f"forward misses 10 u sum|w f| (needs {ratio:.3f})"
    return ratio


def check_bwd(gp2, gd2, c):
    """grad_points2: |err| <= (n_e + 8) u sum|terms|; grad_d2: finite and |err| <= (D2 + 16) u T_e."""
    r = interp_bwd64(c["g"], c["points2"], c["idx"], c["d2"], c["D1"])
    gp2, gd2 = np.asarray(gp2, np.float64), np.asarray(gd2, np.float64)
    assert gp2.shape == r["gp2"].shape and gd2.shape == r["gd2"].shape
    assert np.isfinite(gd2).all() and np.isfinite(gp2).all()
    err = np.abs(gp2 - r["gp2"])
    n = r["n2"][..., None]
    over = err - (n + C_GP2) * U * r["ap2"]
    need = float(((err / (U * np.where(r["ap2"] > 0, r["ap2"], 1.0))) - n).max())
    print(f"grad_points2: max err {err.max():.3e}, max n_e {int(n.max())}, needs n_e + {need:.3f}")
    assert (over <= 0).all(), f"grad_points2 misses (n_e + 8) u sum|terms| (needs n_e + {need:.3f})"
    D2 = c["points2"].shape[2]
    ratio = _worst(np.abs(gd2 - r["gd2"]), r["Te"], "grad_d2", "D2 + C")
    assert ratio <= D2 + C_GD2, f"grad_d2 misses (D2 + 16) u T_e (needs {ratio:.3f}, D2 = {D2})"
    return need, ratio


# (B, N, S, D2, D1, coincident): every shape with and without skip features, and one case with two coincident coarse points
CASES = [s + (d1, False) for s in KERNEL_SHAPES for d1 in D1S] + [(2, 96, 24, 20, 6, True)]


# ---------------- the golden layers (tests/golden/fp.npz) ----------------

MSG = dict(npoint=32, radius_list=[0.25, 0.5], nsample_list=[8, 16])


def sd_of(gold, tag):
    """The state dict stored under <tag>_sd_*."""
    return {k[len(tag) + 4:]: v for k, v in gold.items() if k.startswith(tag + "_sd_")}


def bcn(a):
    """[B,N,C] -> contiguous [B,C,N] (None stays None)."""
    return None if a is None else np.ascontiguousarray(a.transpose(0, 2, 1))


def fp_ref_layer(gold, tag, dtype):
    return fp_layer(sd_of(gold, tag), bcn(gold[f"{tag}_xyz1"]), bcn(gold[f"{tag}_xyz2"]), bcn(gold.get(f"{tag}_points1")),
                    bcn(gold[f"{tag}_points2"]), dtype, gold[f"{tag}_g_out"])


def msg_ref_layer(gold, dtype):
    return msg_layer(sd_of(gold, "msg"), bcn(gold["msg_xyz"]), bcn(gold["msg_points"]), gold["msg_start"], MSG["npoint"],
                     MSG["radius_list"], MSG["nsample_list"], dtype, gold["msg_g_out"], gold["msg_g_xyz"])
