"""Plain restatements of the set-abstraction contracts of csrc/group.hip (include/ured_hip.h):
farthest-point sampling, ball query, grouping in numpy, fp32 with the stated operation order
(float64 for the gradient sums), and one PointNetSetAbstraction layer in torch on the CPU at a
chosen precision. tests/golden/group.npz pins them to the reference's pointnet2_utils.py."""
import numpy as np

F32 = np.float32


def sqd(p, c):
    """((dx*dx) + (dy*dy)) + (dz*dz) in fp32, dx = p.x - c.x; p [..., 3], c broadcastable."""
    p, c = np.asarray(p, F32), np.asarray(c, F32)
    dx, dy, dz = p[..., 0] - c[..., 0], p[..., 1] - c[..., 1], p[..., 2] - c[..., 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def fps(xyz, start, npoint):
    """xyz [B,N,3] fp32, start [B] -> int32 [B,npoint]."""
    xyz = np.asarray(xyz, F32)
    B, N, _ = xyz.shape
    out = np.zeros((B, npoint), np.int32)
    for b in range(B):
        dmin = np.full(N, 1e10, F32)
        f = int(min(max(int(start[b]), 0), N - 1))
        for i in range(npoint):
            out[b, i] = f
            d = sqd(xyz[b], xyz[b, f])
            m = d < dmin
            dmin[m] = d[m]
            f = int(np.argmax(dmin))              # the first (lowest-index) maximum
    return out


def radius2(radius):
    """The squared radius as the comparison sees it: radius ** 2 rounded to fp32."""
    return F32(float(radius) * float(radius))


def ball_query(xyz, new_xyz, r2, nsample):
    """-> int32 [B,S,nsample]: the first nsample j, ascending, with !(d > r2); padded with the first;
    N everywhere in a row without a hit."""
    xyz, new_xyz, r2 = np.asarray(xyz, F32), np.asarray(new_xyz, F32), F32(r2)
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    out = np.full((B, S, nsample), N, np.int32)
    for b in range(B):
        d = sqd(xyz[b][None, :, :], new_xyz[b][:, None, :])          # [S,N]
        hit = ~(d > r2)
        for s in range(S):
            j = np.nonzero(hit[s])[0][:nsample]
            if j.size:
                out[b, s, :j.size] = j
                out[b, s, j.size:] = j[0]
    return out


def group_fwd(xyz, new_xyz, points, idx):
    """-> [B*S*K, C]: columns xyz[idx] - new_xyz[s] (if xyz is given), then points[idx]; zero rows
    for indices outside [0,N)."""
    idx = np.asarray(idx)
    B, S, K = idx.shape
    N = (xyz if xyz is not None else points).shape[1]
    ok = (idx >= 0) & (idx < N)
    ii = np.where(ok, idx, 0)
    bb = np.arange(B)[:, None, None]
    cols = []
    if xyz is not None:
        cols.append(np.asarray(xyz, F32)[bb, ii] - np.asarray(new_xyz, F32)[:, :, None, :])
    if points is not None:
        cols.append(np.asarray(points, F32)[bb, ii])
    out = np.where(ok[..., None], np.concatenate(cols, axis=-1), F32(0))
    return out.reshape(B * S * K, -1).astype(F32)


def group_bwd(g, idx, N, c3):
    """g [B*S*K, C] -> dict of float64 sums (gx [B,N,3] | None, gn [B,S,3] | None, gp [B,N,D] | None),
    and per output element the sum of |terms| (ax, an, ap) and the number of terms (nx: [B,N] for gx /
    gp, K-hits [B,S] for gn): the inputs of the sequential-summation error bound."""
    idx = np.asarray(idx)
    B, S, K = idx.shape
    C = g.shape[1]
    D = C - c3
    g64 = np.asarray(g, np.float64).reshape(B, S, K, C)
    ok = (idx >= 0) & (idx < N)
    full, afull = np.zeros((B, N, C)), np.zeros((B, N, C))
    cnt = np.zeros((B, N), np.int64)
    for b in range(B):
        j = idx[b][ok[b]]
        np.add.at(full[b], j, g64[b][ok[b]])
        np.add.at(afull[b], j, np.abs(g64[b][ok[b]]))
        np.add.at(cnt[b], j, 1)
    r = dict(n=cnt, gx=None, gn=None, gp=None, ax=None, an=None, ap=None, nn=ok.sum(-1))
    if c3:
        gm = g64[..., :3] * ok[..., None]
        r.update(gx=full[..., :3], ax=afull[..., :3], gn=-gm.sum(2), an=np.abs(gm).sum(2))
    if D:
        r.update(gp=full[..., c3:], ap=afull[..., c3:])
    return r


def sa_layer(sd, xyz, points, start, npoint, radius, nsample, group_all, dtype, g_out, g_xyz, eps=1e-5,
             momentum=0.1):
    """One PointNetSetAbstraction layer in training mode, restated with plain torch ops on the CPU
    at `dtype` (sampling and ball query by the fp32 contracts above). sd: the layer's state dict
    (numpy); xyz [B,3,N], points [B,D,N] | None; the loss is sum(out * g_out) + sum(new_xyz * g_xyz).
    -> dict: new_xyz [B,3,S], out [B,C,S], gxyz, gpoints, grads {name: array}, running stats
    {name: array}, pre (the BN outputs of every layer, [B,S,K,C_i]), fps_idx, idx."""
    import torch
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x = T(xyz).requires_grad_(True)
    p = None if points is None else T(points).requires_grad_(True)
    B, _, N = x.shape
    xt = x.permute(0, 2, 1)
    pt = None if p is None else p.permute(0, 2, 1)
    fi = idx = None
    if group_all:
        new_xyz = torch.zeros(B, 1, 3, dtype=dtype)
        rows = (xt if pt is None else torch.cat([xt, pt], -1))[:, None]
    else:
        x32 = np.ascontiguousarray(np.asarray(xyz, F32).transpose(0, 2, 1))
        fi = fps(x32, start, npoint)
        bb = np.arange(B)[:, None]
        idx = ball_query(x32, x32[bb, fi], radius2(radius), nsample)
        fl, il = torch.from_numpy(fi.astype(np.int64)), torch.from_numpy(idx.astype(np.int64))
        bt = torch.arange(B)
        new_xyz = xt[bt[:, None], fl]
        rows = xt[bt[:, None, None], il] - new_xyz[:, :, None, :]
        if pt is not None:
            rows = torch.cat([rows, pt[bt[:, None, None], il]], -1)
    L = len([k for k in sd if k.startswith("mlp_convs.") and k.endswith(".weight")])
    params, pres, running = {}, [], {}
    h = rows
    for i in range(L):
        W = T(sd[f"mlp_convs.{i}.weight"]).requires_grad_(True)
        bias = T(sd[f"mlp_convs.{i}.bias"]).requires_grad_(True)
        gamma = T(sd[f"mlp_bns.{i}.weight"]).requires_grad_(True)
        beta = T(sd[f"mlp_bns.{i}.bias"]).requires_grad_(True)
        params.update({f"mlp_convs.{i}.weight": W, f"mlp_convs.{i}.bias": bias, f"mlp_bns.{i}.weight": gamma,
                       f"mlp_bns.{i}.bias": beta})
        y = h @ W.view(W.shape[0], -1).t() + bias
        mean = y.mean((0, 1, 2))
        var = ((y - mean) ** 2).mean((0, 1, 2))
        pre = (y - mean) / torch.sqrt(var + eps) * gamma + beta
        pres.append(pre.detach().numpy())
        h = torch.relu(pre)
        n = y.numel() // y.shape[-1]
        running[f"mlp_bns.{i}.running_mean"] = ((1 - momentum) * T(sd[f"mlp_bns.{i}.running_mean"])
                                                + momentum * mean.detach()).numpy()
        running[f"mlp_bns.{i}.running_var"] = ((1 - momentum) * T(sd[f"mlp_bns.{i}.running_var"])
                                               + momentum * var.detach() * n / (n - 1)).numpy()
    out = h.max(2)[0].permute(0, 2, 1)
    nx = new_xyz.permute(0, 2, 1)
    loss = (out * T(g_out)).sum()
    if not group_all:
        loss = loss + (nx * T(g_xyz)).sum()
    ins = [x] + ([] if p is None else [p])
    gr = torch.autograd.grad(loss, ins + list(params.values()))
    return dict(new_xyz=nx.detach().numpy(), out=out.detach().numpy(), gxyz=gr[0].numpy(),
                gpoints=None if p is None else gr[1].numpy(),
                grads={k: v.numpy() for k, v in zip(params, gr[len(ins):])}, running=running, pre=pres,
                fps_idx=fi, idx=idx)


def decision_margin(pres):
    """The smallest |BN output| over all layers (a ReLU decision) and the smallest gap between a
    positive max-pool winner of the last layer and the next smaller value of its group (equal values
    come from identical rows and decide nothing)."""
    relu_m = min(float(np.abs(p).min()) for p in pres)
    a = np.maximum(pres[-1], 0.0)                                   # [B,S,K,C]
    srt = -np.sort(-a, axis=2)
    top = srt[:, :, :1, :]
    below = np.where(srt < top, srt, -np.inf).max(2)                # next smaller value, -inf if none
    gap = np.where(top[:, :, 0, :] > 0, top[:, :, 0, :] - below, np.inf)
    return relu_m, float(gap.min())
