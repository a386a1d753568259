"""Plain torch restatement of the 3D-GCN contracts (include/ured_hip.h, ured_hip/gcn.py,
network/P_3DGC.py, network/gc3d_encoder.py), runnable in float64 and float32 on the CPU. The kernel
level is written out explicitly (winning slots with the lowest-slot tie rule, both gradients); the
modules and the encoder are compositions of those pieces under autograd. Nothing here touches the
device library."""
import numpy as np
import torch
import torch.nn.functional as F

# ---------------- kernel level ----------------


def dirs(vertices, idx):
    """vertices [B,V,3], idx [B,V,n] -> [B,V,n,3]: (v[idx] - v) / max(|.|, 1e-12)."""
    B, V, n = idx.shape
    nb = vertices[torch.arange(B).view(B, 1, 1), idx.long()]
    d = nb - vertices.unsqueeze(2)
    return d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def _theta(dirn, sdn, S):
    """-> relu(dirn . sdn) [B,V,n,S,C] and the raw dot products."""
    B, V, n, _ = dirn.shape
    C = sdn.shape[1] // S
    raw = ((dirn[..., 0:1] * sdn[0]) + (dirn[..., 1:2] * sdn[1])) + (dirn[..., 2:3] * sdn[2])
    raw = raw.view(B, V, n, S, C)
    return torch.relu(raw), raw                            # relu: no gradient at 0 (clamp_min passes one)


def _products(dirn, sdn, feat, idx, S):
    B, V, n, _ = dirn.shape
    C = sdn.shape[1] // S
    th, raw = _theta(dirn, sdn, S)
    if feat is None:
        return th, th, None, raw
    sup = feat.view(B, V, S + 1, C)[:, :, 1:]                                   # [B,V,S,C]
    gathered = sup[torch.arange(B).view(B, 1, 1), idx.long()]                   # [B,V,n,S,C]
    return th * gathered, th, gathered, raw


def _lowest_argmax(p):
    """p [B,V,n,...] -> (max over dim 2, the lowest index that attains it)."""
    best, slot = p[:, :, 0], torch.zeros(p[:, :, 0].shape, dtype=torch.long)
    for j in range(1, p.shape[2]):
        up = p[:, :, j] > best
        best = torch.where(up, p[:, :, j], best)
        slot = torch.where(up, torch.full_like(slot, j), slot)
    return best, slot


def conv_fwd(dirn, sdn, feat, idx, S):
    """-> out [B*V, C], slot long [B*V, S, C] (feat [B*V, (S+1)*C] or None)."""
    B, V, n, _ = dirn.shape
    C = sdn.shape[1] // S
    prod = _products(dirn, sdn, feat, idx, S)[0]
    best, slot = _lowest_argmax(prod)                                           # [B,V,S,C]
    acc = best[:, :, 0]
    for s in range(1, S):
        acc = acc + best[:, :, s]
    if feat is not None:
        acc = feat.view(B, V, S + 1, C)[:, :, 0] + acc
    return acc.reshape(B * V, C), slot.reshape(B * V, S, C)


def conv_bwd(g, dirn, sdn, feat, idx, slot, S):
    """-> grad_feat [B*V, (S+1)*C] (None without feat), grad_sdn [3, S*C]; relu passes iff theta > 0."""
    B, V, n, _ = dirn.shape
    C = sdn.shape[1] // S
    prod, th, gathered, raw = _products(dirn, sdn, feat, idx, S)
    sl = slot.view(B, V, 1, S, C)
    pick = lambda t: torch.gather(t, 2, sl).squeeze(2)                          # noqa: E731  [B,V,S,C]
    th_w, raw_w = pick(th), pick(raw)
    gg = g.view(B, V, 1, C).expand(B, V, S, C)
    f_w = pick(gathered) if feat is not None else torch.ones_like(th_w)
    w = torch.where(raw_w > 0, gg * f_w, torch.zeros_like(gg))                  # [B,V,S,C]
    d_w = torch.gather(dirn.view(B, V, n, 1, 1, 3).expand(B, V, n, S, C, 3), 2,
                       sl.unsqueeze(-1).expand(B, V, 1, S, C, 3)).squeeze(2)    # [B,V,S,C,3]
    gsdn = (w.unsqueeze(-1) * d_w).sum(dim=(0, 1)).permute(2, 0, 1).reshape(3, S * C)
    if feat is None:
        return None, gsdn
    gfeat = torch.zeros(B, V, S + 1, C, dtype=g.dtype)
    gfeat[:, :, 0] = g.view(B, V, C)
    rows = torch.gather(idx.long().view(B, V, n, 1, 1).expand(B, V, n, S, C), 2, sl).squeeze(2)   # [B,V,S,C]
    ok = (rows >= 0) & (rows < V)
    tgt = gfeat[:, :, 1:]                                                       # [B,V,S,C] view
    bi = torch.arange(B).view(B, 1, 1, 1).expand(B, V, S, C)
    si = torch.arange(S).view(1, 1, S, 1).expand(B, V, S, C)
    ci = torch.arange(C).view(1, 1, 1, C).expand(B, V, S, C)
    tgt.index_put_((bi[ok], rows[ok], si[ok], ci[ok]), (gg * th_w)[ok], accumulate=True)
    return gfeat.reshape(B * V, (S + 1) * C), gsdn


def pool_fwd(feat, idx, sample):
    """feat [B*V, C], idx [B,V,k], sample [P] -> out [B*P, C], slot long [B*P, C]."""
    B, V, k = idx.shape
    C = feat.shape[1]
    rows = idx.long()[:, sample.long()]                                         # [B,P,k]
    vals = feat.view(B, V, C)[torch.arange(B).view(B, 1, 1), rows]              # [B,P,k,C]
    best, slot = _lowest_argmax(vals)
    return best.reshape(-1, C), slot.reshape(-1, C)


def pool_bwd(g, idx, sample, slot, V):
    B, _, k = idx.shape
    C = g.shape[1]
    P = sample.shape[0]
    rows = idx.long()[:, sample.long()]                                         # [B,P,k]
    win = torch.gather(rows.unsqueeze(-1).expand(B, P, k, C), 2, slot.view(B, P, 1, C)).squeeze(2)   # [B,P,C]
    out = torch.zeros(B, V, C, dtype=g.dtype)
    bi = torch.arange(B).view(B, 1, 1).expand(B, P, C)
    ci = torch.arange(C).view(1, 1, C).expand(B, P, C)
    out.index_put_((bi, win, ci), g.view(B, P, C), accumulate=True)
    return out.reshape(B * V, C)


class _Conv(torch.autograd.Function):
    """conv_fwd / conv_bwd under autograd (differentiable in sdn and feat)."""

    @staticmethod
    def forward(ctx, dirn, sdn, feat, idx, S):
        out, slot = conv_fwd(dirn, sdn, feat, idx, S)
        ctx.save_for_backward(dirn, sdn, feat, idx, slot)
        ctx.S = S
        return out

    @staticmethod
    def backward(ctx, g):
        dirn, sdn, feat, idx, slot = ctx.saved_tensors
        gf, gs = conv_bwd(g, dirn, sdn, feat, idx, slot, ctx.S)
        return None, gs, gf, None, None


# ---------------- kernel-level test inputs ----------------

KERNEL_CASES = [  # (B, V, n, S, C): every value of every dimension, the extremes together, sizes across a tile
    (1, 5, 1, 1, 1), (2, 5, 4, 3, 8), (1, 5, 10, 7, 100), (2, 5, 4, 7, 128),
    (2, 33, 1, 3, 128), (1, 33, 4, 7, 1), (2, 33, 10, 1, 8), (1, 33, 10, 3, 100),
    (1, 130, 1, 7, 8), (2, 130, 4, 1, 100), (1, 130, 10, 3, 1), (2, 130, 10, 7, 128),
    (2, 130, 4, 3, 128), (1, 33, 4, 1, 128),
]


def kernel_case(case, seed, layer):
    """Inputs of one GcnConvFn case (float64 tensors): dirn and sdn entries are multiples of 1/8 in
    [-1, 1] and feat entries multiples of 1/8 in [-4, 4], so every theta and every product is exact
    in fp32: every ReLU and max decision is the same in fp32 and float64, and a tie is a tie in both
    (the lowest slot wins it). Vertex 0's directions are zero (every theta is 0) and vertex 1 has
    every theta of support 0 <= 0; index 0 is shared by half of the entries. g is continuous."""
    B, V, n, S, C = case
    rng = np.random.default_rng(seed)
    dirn = rng.integers(-8, 9, size=(B, V, n, 3)) / 8.0
    sdn = rng.integers(-8, 9, size=(3, S * C)) / 8.0
    dirn[:, 0] = 0.0                                       # vertex 0: every theta is 0 -> max 0, no gradient
    if V > 1:
        dirn[:, 1] = -np.abs(dirn[:, 1])                   # vertex 1 against a non-negative column block
        sdn[:, :C] = np.abs(sdn[:, :C])                    # support 0: thetas of vertex 1 all <= 0
    idx = rng.integers(0, V, size=(B, V, n))
    idx[rng.random((B, V, n)) < 0.5] = 0                   # one row that many vertices share
    feat = rng.integers(-32, 33, size=(B * V, (S + 1) * C)) / 8.0 if layer else None
    g = rng.standard_normal((B * V, C))
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    return t(dirn), t(sdn), t(feat), t(idx.astype(np.int32)), t(g)


def winner_gaps(dirn, sdn, feat, idx, S):
    """-> (the least winner - runner-up over the maxima that are neither an exact 0 nor an exact
    tie, the number of exact ties at a non-zero maximum, max |product|, the number of theta == 0,
    whether every product is exactly representable in fp32)."""
    prod, _, _, raw = _products(dirn, sdn, feat, idx, S)
    n = prod.shape[2]
    mx = prod.abs().max().item()
    nzero = int((raw == 0).sum())
    exact = bool((prod.float().double() == prod.double()).all())
    if n == 1:
        return float("inf"), 0, mx, nzero, exact
    top = torch.topk(prod, 2, dim=2)[0]
    gap = top[:, :, 0] - top[:, :, 1]
    live = top[:, :, 0] != 0
    ties = int((live & (gap == 0)).sum())
    sel = gap[live & (gap > 0)]
    return (sel.min().item() if sel.numel() else float("inf")), ties, mx, nzero, exact


# ---------------- module level ----------------

def knn_index(p1, p2, K):
    """The K nearest p2 rows of every p1 row by the direct distance, sorted by (distance, index)
    -> long [B,n,K] and the sorted distances [B,n,m]."""
    d = p1.unsqueeze(2) - p2.unsqueeze(1)
    d = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
    ds, order = torch.sort(d, dim=-1, stable=True)
    return order[..., :K], ds


def get_neighbor_index(vertices, neighbor_num):
    return knn_index(vertices, vertices, neighbor_num + 1)[0][:, :, 1:]


def get_nearest_index(target, source):
    return knn_index(target, source, 1)[0]


def conv_surface(directions, S, neighbor_index, vertices):
    B, V, n = neighbor_index.shape
    out = _Conv.apply(dirs(vertices, neighbor_index), F.normalize(directions, dim=0), None, neighbor_index, S)
    return out.view(B, V, -1)


def conv_layer(weights, bias, directions, S, neighbor_index, vertices, feature_map):
    B, V, n = neighbor_index.shape
    feat = feature_map.reshape(B * V, -1) @ weights + bias
    out = _Conv.apply(dirs(vertices, neighbor_index), F.normalize(directions, dim=0), feat, neighbor_index, S)
    return out.view(B, V, -1)


def pool_layer(vertices, feature_map, sample_idx, neighbor_num=4):
    """sample_idx: the torch.randperm(vertice_num)[:pool_num] of the layer."""
    B, V, C = feature_map.shape
    idx = get_neighbor_index(vertices, neighbor_num)
    nb = feature_map[torch.arange(B).view(B, 1, 1), idx]                        # [B,V,k,C]
    pooled = nb.max(dim=2)[0]
    return vertices[:, sample_idx], pooled[:, sample_idx]


def _bn(x, P, name, training, stats):
    """BatchNorm1d on [M, C]; stats: dict of running buffers, updated in place when training."""
    return F.batch_norm(x, stats[name + ".running_mean"], stats[name + ".running_var"], P[name + ".weight"],
                        P[name + ".bias"], training, 0.1, 1e-5)


def encoder(P, vertices, training, samples, n_num=10, S=7):
    """GCN3D_ENCODER as a function of its state_dict P (tensors of vertices' dtype; the running
    statistics are cloned and the updated ones returned). samples: the two randperm prefixes.
    -> f_global [B,256], feat [B,256,V], stats."""
    stats = {k: v.clone() for k, v in P.items() if "running_" in k}
    B, V, _ = vertices.shape

    def layer(i, ni, v, fm):
        return conv_layer(P[f"conv_{i}.weights"], P[f"conv_{i}.bias"], P[f"conv_{i}.directions"], S, ni, v, fm)

    def bn_relu(name, fm):
        b, v, c = fm.shape
        return F.relu(_bn(fm.reshape(b * v, c), P, name, training, stats)).view(b, v, c)

    ni = get_neighbor_index(vertices, n_num)
    fm_0 = F.relu(conv_surface(P["conv_0.directions"], S, ni, vertices))
    fm_1 = bn_relu("bn1", layer(1, ni, vertices, fm_0))
    v1, fp1 = pool_layer(vertices, fm_1, samples[0])
    ni = get_neighbor_index(v1, min(n_num, v1.shape[1] // 8))
    fm_2 = bn_relu("bn2", layer(2, ni, v1, fp1))
    fm_3 = bn_relu("bn3", layer(3, ni, v1, fm_2))
    v2, fp2 = pool_layer(v1, fm_3, samples[1])
    ni = get_neighbor_index(v2, min(n_num, v2.shape[1] // 8))
    fm_4 = layer(4, ni, v2, fp2)
    f_global = fm_4.max(1)[0]
    n1 = get_nearest_index(vertices, v1).squeeze(2)
    n2 = get_nearest_index(vertices, v2).squeeze(2)
    bi = torch.arange(B).view(B, 1)
    x = torch.cat([fm_0, fm_1, fm_2[bi, n1], fm_3[bi, n1], fm_4[bi, n2]], dim=2).reshape(B * V, -1)
    for conv, bn in (("conv1d_block.0", "conv1d_block.1"), ("conv1d_block.3", "conv1d_block.4")):
        x = x @ P[conv + ".weight"].squeeze(-1).t() + P[conv + ".bias"]
        x = F.relu(_bn(x, P, bn, training, stats))
    return f_global, x.view(B, V, -1).permute(0, 2, 1), stats


# ---------------- the conditions the goldens are searched for ----------------

def kernel_case_ok(case, seed, layer):
    dirn, sdn, feat, idx, _ = kernel_case(case, seed, layer)
    gap, _, mx, nzero, exact = winner_gaps(dirn, sdn, feat, idx, case[3])
    return nzero > 0 and exact and gap > 1e-5 * mx


def sorted_gaps_ok(ds, ranks, eps=1e-6):
    """ds: sorted distances [..., m]; the first `ranks` of every row differ pairwise by more than eps."""
    d = ds[..., :min(ranks, ds.shape[-1])]
    return d.shape[-1] < 2 or bool(((d[..., 1:] - d[..., :-1]) > eps).all())


def cloud_ok(vertices, n):
    """Every K-NN row's sorted float64 distances through rank n + 2 are separated by more than 1e-6."""
    return sorted_gaps_ok(knn_index(vertices, vertices, 1)[1], n + 3)


def layer_case_ok(weights, bias, directions, S, idx, vertices, feature_map):
    B, V, n = idx.shape
    feat = feature_map.reshape(B * V, -1) @ weights + bias
    dirn, sdn = dirs(vertices, idx), F.normalize(directions, dim=0)
    gap, ties, mx, _, _ = winner_gaps(dirn, sdn, feat, idx, S)
    raw = _theta(dirn, sdn, S)[1]
    return bool(raw.abs().min() > 2e-6) and ties == 0 and gap > 1e-5 * mx


def encoder_samples(V, rseed):
    """The two torch.randperm prefixes that a forward seeded with torch.manual_seed(rseed) draws."""
    state = torch.get_rng_state()
    torch.manual_seed(rseed)
    s0 = torch.randperm(V)[:V // 4]
    s1 = torch.randperm(V // 4)[:V // 16]
    torch.set_rng_state(state)
    return s0, s1


def encoder_clouds_ok(vertices, rseed, n_num=10):
    V = vertices.shape[1]
    s0, s1 = encoder_samples(V, rseed)
    v1 = vertices[:, s0]
    v2 = v1[:, s1]
    return (cloud_ok(vertices, n_num) and cloud_ok(v1, max(min(n_num, v1.shape[1] // 8), 4))
            and cloud_ok(v2, min(n_num, v2.shape[1] // 8))
            and sorted_gaps_ok(knn_index(vertices, v1, 1)[1], 2) and sorted_gaps_ok(knn_index(vertices, v2, 1)[1], 2))


def encoder_params(seed, S=7):
    """A GCN3D_ENCODER state_dict (float64 tensors, the reference's keys and shapes) from a seed:
    uniform weights at the initialisation's scale, BatchNorm weights, biases and running statistics
    away from their defaults."""
    rng = np.random.default_rng(seed)
    P = {}
    u = lambda a, *shape: torch.from_numpy(rng.uniform(-a, a, shape))           # noqa: E731

    def bn(name, c):
        P[name + ".weight"] = torch.from_numpy(rng.uniform(0.5, 1.5, c))
        P[name + ".bias"] = u(0.2, c)
        P[name + ".running_mean"] = u(0.2, c)
        P[name + ".running_var"] = torch.from_numpy(rng.uniform(0.5, 1.5, c))
        P[name + ".num_batches_tracked"] = torch.tensor(3)

    P["conv_0.directions"] = u(1 / np.sqrt(S * 128), 3, S * 128)
    for i, (cin, cout) in enumerate([(128, 128), (128, 256), (256, 256), (256, 256)], start=1):
        a = 1 / np.sqrt(cout * (S + 1))
        P[f"conv_{i}.weights"] = u(a, cin, (S + 1) * cout)
        P[f"conv_{i}.bias"] = u(a, (S + 1) * cout)
        P[f"conv_{i}.directions"] = u(a, 3, S * cout)
    bn("bn1", 128), bn("bn2", 256), bn("bn3", 256)
    for i, (cin, cout) in ((0, (1024, 512)), (3, (512, 256))):
        P[f"conv1d_block.{i}.weight"] = u(1 / np.sqrt(cin), cout, cin, 1)
        P[f"conv1d_block.{i}.bias"] = u(1 / np.sqrt(cin), cout)
        bn(f"conv1d_block.{i + 1}", cout)
    return P


def cast(P, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in P.items()}
