"""Float64 restatements of the graph-node kernels: csrc/node.hip (node GEMM with its epilogue,
column sums, BatchNorm1d over node sets with its SyncBN modes) and csrc/attn.hip (multi-head softmax
attention, forward and backward); contracts in include/ured_hip.h. Shared by
tests/test_node_kernels_gpu.py and tests/test_attn_kernels_gpu.py. Plain torch on the CPU, no
fixtures, no import of ured_hip. tests/test_node_ref.py pins every function here to an independent
torch composition (torch.nn.BatchNorm1d with autograd, autograd through
attention_graph.attention.softmax_attention), so the GPU tests compare kernels with arithmetic
that has a check of its own.

Every function takes `dtype` (float64 by default): the GPU tests run the same restatement in
float32 to measure how far fp32 arithmetic alone moves a result (their tolerance's first term).

Conventions
  * GEMM operands are the mathematical matrices: A [M, K] (optionally cat([A, A2], 1), A [M, k1]),
    B [K, N] (optionally the column blocks cat([B, B2], 1), B [K, n1]); how the kernel addresses
    them (element strides) is the test's business;
  * node sets: rows [off[s], off[s+1]) of Y are one call of the BatchNorm module;
  * per-rank statistics / sums are [3, N] float64: (count, mean, M2) forward, (sum g, sum g*xhat,
    count) backward, the layouts of stats_out / sums_out;
  * attention tensors are node-major [B, nodes, H*d], channel h*d + j = head h, component j.
"""
import torch

F64 = torch.float64


def _c(t, dtype):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", dtype)


# ---- node GEMM -----------------------------------------------------------------------------

def gemm(A, B, *, A2=None, B2=None, bias=None, rowbias=None, rdiv=1, relu=False, gate=None, R=None, R_ncols=None,
         C_old=None, dtype=F64):
    """One node-GEMM job in the kernel's epilogue order:
    v = acc + bias[n] + rowbias[m // rdiv, n]; ReLU; gate[m, n] > 0 ? v : 0; + R[m, n] for
    n < R_ncols; + C_old (accumulate). A may be None (k1 = 0: every k comes from A2)."""
    A, A2, B, B2 = _c(A, dtype), _c(A2, dtype), _c(B, dtype), _c(B2, dtype)
    k1 = 0 if A is None else A.shape[1]
    M = A2.shape[0] if A is None else A.shape[0]
    blocks = []
    for Bb in (B, B2):                       # the column blocks, each from the K-split A
        if Bb is None:
            continue
        acc = torch.zeros(M, Bb.shape[1], dtype=dtype)
        if A is not None and k1 > 0:
            acc = acc + A @ Bb[:k1]
        if A2 is not None and A2.shape[1] > 0:
            acc = acc + A2 @ Bb[k1:]
        blocks.append(acc)
    v = torch.cat(blocks, 1)
    N = v.shape[1]
    if bias is not None:
        v = v + _c(bias, dtype)
    if rowbias is not None:
        v = v + _c(rowbias, dtype)[torch.arange(M) // rdiv]
    if relu:
        v = v.clamp(min=0)
    if gate is not None:
        v = torch.where(_c(gate, dtype) > 0, v, torch.zeros_like(v))
    if R is not None:
        nc = N if R_ncols is None else R_ncols
        v = v.clone()
        v[:, :nc] += _c(R, dtype)[:, :nc]
    if C_old is not None:
        v = v + _c(C_old, dtype)
    return v


def colsum(g, c_old=None, accumulate=False, dtype=F64):
    """C[n] (+)= sum_m g[m, n] (zero rows: zeros, or C unchanged)."""
    s = _c(g, dtype).sum(0)
    return s + _c(c_old, dtype) if accumulate else s


# ---- BatchNorm1d over node sets --------------------------------------------------------------

def bn_sets(Y, off, gamma, beta, running_mean, running_var, momentum, eps, training, relu_in, num_batches_tracked=0,
            dtype=F64):
    """-> dict(act [R, N], mean / invstd [S, N], running_mean, running_var, num_batches_tracked).
    Training: batch statistics per set (biased variance normalises, the unbiased one updates the
    running variance), running statistics updated in set order; eval: the running statistics."""
    Y, gamma, beta = _c(Y, dtype), _c(gamma, dtype), _c(beta, dtype)
    rm, rv = _c(running_mean, dtype).clone(), _c(running_var, dtype).clone()
    x = Y.clamp(min=0) if relu_in else Y
    act, means, invstds = torch.empty_like(Y), [], []
    nbt = int(num_batches_tracked)
    for a, b in zip(off[:-1], off[1:]):
        xs, cnt = x[a:b], b - a
        if training:
            mu = xs.sum(0) / cnt
            var = ((xs - mu) ** 2).sum(0) / cnt
            rm = (1 - momentum) * rm + momentum * mu
            rv = (1 - momentum) * rv + momentum * (var * cnt / (cnt - 1) if cnt > 1 else var)
            nbt += 1
        else:
            mu, var = rm, rv
        inv = 1.0 / torch.sqrt(var + eps)
        act[a:b] = (xs - mu) * inv * gamma + beta
        means.append(mu)
        invstds.append(inv)
    return {"act": act, "mean": torch.stack(means), "invstd": torch.stack(invstds), "running_mean": rm,
            "running_var": rv, "num_batches_tracked": nbt}


def bn_sets_bwd(G, Y, off, gamma, mean, invstd, training, relu_in, dtype=F64):
    """-> (dY, dgamma, dbeta). Training: dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat))
    per set; eval: dx = gamma * invstd * g. relu_in: dY masked by Y > 0. dgamma / dbeta summed over
    the sets (one module)."""
    G, Y, gamma, mean, invstd = (_c(t, dtype) for t in (G, Y, gamma, mean, invstd))
    x = Y.clamp(min=0) if relu_in else Y
    dY = torch.empty_like(Y)
    dgamma, dbeta = torch.zeros_like(gamma), torch.zeros_like(gamma)
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        g, xh, cnt = G[a:b], (x[a:b] - mean[s]) * invstd[s], b - a
        sg, sgx = g.sum(0), (g * xh).sum(0)
        dgamma, dbeta = dgamma + sgx, dbeta + sg
        dx = gamma * invstd[s] * ((g - sg / cnt - xh * (sgx / cnt)) if training else g)
        dY[a:b] = torch.where(Y[a:b] > 0, dx, torch.zeros_like(dx)) if relu_in else dx
    return dY, dgamma, dbeta


def bn_rank_stats(Y, relu_in, dtype=F64):
    """One rank's rows of one set -> [3, N] (count, mean, M2 about that mean)."""
    Y = _c(Y, dtype)
    x = Y.clamp(min=0) if relu_in else Y
    cnt = x.shape[0]
    mu = x.sum(0) / max(cnt, 1)
    return torch.stack([torch.full_like(mu, float(cnt)), mu, ((x - mu) ** 2).sum(0)])


def merge_stats(a, b):
    """Chan's merge of two (count, mean, M2) triples [3, N]."""
    na, nb = a[0], b[0]
    n = na + nb
    delta = b[1] - a[1]
    safe = n.clamp(min=1)
    return torch.stack([n, a[1] + delta * nb / safe, a[2] + b[2] + delta * delta * na * nb / safe])


def stats_to_bn(st, eps):
    """Merged (count, mean, M2) -> (mean, invstd, unbiased variance) as the stats_in forward uses
    them."""
    c, mu, var = st[0], st[1], st[2] / st[0].clamp(min=1)
    unb = torch.where(c > 1, var * c / (c - 1).clamp(min=1), var)
    return mu, 1.0 / torch.sqrt(var + eps), unb


def bn_rank_sums(G, Y, mean, invstd, relu_in, dtype=F64):
    """One rank's rows of one set -> [3, N] (sum g, sum g * xhat, count); mean / invstd [N] are
    the set's (merged) statistics."""
    G, Y, mean, invstd = (_c(t, dtype) for t in (G, Y, mean, invstd))
    x = Y.clamp(min=0) if relu_in else Y
    xh = (x - mean) * invstd
    sg = G.sum(0)
    return torch.stack([sg, (G * xh).sum(0), torch.full_like(sg, float(G.shape[0]))])


# ---- attention -----------------------------------------------------------------------------

def _heads(t, H):
    B, n, C = t.shape
    return t.view(B, n, H, C // H).permute(0, 2, 1, 3)          # [B, H, n, d]


def _nodes(t):
    B, H, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, n, H * d)


def attn_fwd(q, k, v, H, scale, dtype=F64):
    """q [B, n, H*d], k / v [B, m, H*d] -> (out [B, n, H*d], P [B, H, n, m]);
    S = q k^T * scale per head, P = exp(S - rowmax) / rowsum, out = P v."""
    q, k, v = (_heads(_c(t, dtype), H) for t in (q, k, v))
    S = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    E = torch.exp(S - S.amax(-1, keepdim=True))
    P = E / E.sum(-1, keepdim=True)
    return _nodes(torch.einsum("bhij,bhjd->bhid", P, v)), P


def attn_bwd(q, k, v, P, dout, H, scale, dtype=F64):
    """-> (dq, dk, dv) from the saved weights P: dV = P^T dO, dP = dO V^T,
    dS = P * (dP - sum_j P dP) * scale, dQ = dS K, dK = dS^T Q."""
    q, k, v, dO = (_heads(_c(t, dtype), H) for t in (q, k, v, dout))
    P = _c(P, dtype)
    dV = torch.einsum("bhij,bhid->bhjd", P, dO)
    dP = torch.einsum("bhid,bhjd->bhij", dO, v)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True)) * scale
    dQ = torch.einsum("bhij,bhjd->bhid", dS, k)
    dK = torch.einsum("bhij,bhid->bhjd", dS, q)
    return _nodes(dQ), _nodes(dK), _nodes(dV)
