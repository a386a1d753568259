"""Float64 restatements of the BatchNorm / max-pool bookkeeping around ured_gemm (csrc/mlp.hip,
csrc/syncbn.hip; contracts in include/ured_hip.h), shared by tests/test_epilogue_gpu.py,
tests/test_bn_glue_gpu.py and tests/test_syncbn_kernels_gpu.py. Plain torch float64 on the CPU, no
fixtures. tests/test_bn_ref.py pins this module to torch.nn.functional.batch_norm + autograd on the
expanded (repeat_interleave) batch, so the GPU tests compare kernels with arithmetic that has an
independent check of its own.

Conventions
  * partials: [2][N][blocks] (one column's block partials contiguous), blocks of BM = 128 rows;
    forward {block mean, M2 about it}, backward {sum g, sum g * xhat};
  * row multiplicities: w_rows [M] says how many identical batch rows each stored row stands for
    (row_weights() expands the kernels' per-group form); None = all ones;
  * activation orders (EPI_BNBWD bwd_res / ured_bn_bwd_apply res):
      ACT_ENC  Conv -> BN -> ReLU   p = y,       g = dh * (y*scale+shift > 0)
      ACT_RES  Conv -> ReLU -> BN   p = relu(y), g = dh, dY masked by (y > 0)
      ACT_BN   Conv -> BN           p = y,       g = dh
    where dh is the gradient arriving at the layer's output, already summed over the copies of a
    stored row.
"""
import torch

BM = 128
ACT_ENC, ACT_RES, ACT_BN = 0, 1, 2
U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)


def nblocks(M):
    return (M + BM - 1) // BM


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)


def row_weights(group_w, group_rows, M):
    """Per-group multiplicities (row r belongs to group r // group_rows) -> per-row [M] float64."""
    if group_w is None:
        return None
    gw = f64(torch.as_tensor(group_w))
    return gw[torch.arange(M) // group_rows]


def block_partials(p, M=None):
    """Forward partials of p [M][N]: out[0][n][b] = mean of block b's valid rows, out[1][n][b] =
    their M2 about that mean."""
    p = f64(p)
    M = p.shape[0] if M is None else M
    out = torch.zeros(2, p.shape[1], nblocks(M), dtype=torch.float64)
    for b in range(nblocks(M)):
        rows = p[b * BM:min(M, (b + 1) * BM)]
        mu = rows.mean(0)
        out[0, :, b] = mu
        out[1, :, b] = ((rows - mu) ** 2).sum(0)
    return out


def block_bwd_partials(g, xhat, M=None):
    """Backward partials: out[0][n][b] = sum g, out[1][n][b] = sum g * xhat over block b's rows."""
    g, xhat = f64(g), f64(xhat)
    M = g.shape[0] if M is None else M
    out = torch.zeros(2, g.shape[1], nblocks(M), dtype=torch.float64)
    for b in range(nblocks(M)):
        sl = slice(b * BM, min(M, (b + 1) * BM))
        out[0, :, b] = g[sl].sum(0)
        out[1, :, b] = (g[sl] * xhat[sl]).sum(0)
    return out


def block_counts(M, group_w=None, group_rows=0):
    """Weighted row count of every 128-row block (a block lies inside one group) and its weight."""
    b = torch.arange(nblocks(M))
    rows = torch.clamp(M - b * BM, max=BM).double()
    w = torch.ones(nblocks(M), dtype=torch.float64) if group_w is None else f64(group_w)[(b * BM) // group_rows]
    return rows * w, w


def merge_partials(ws, M, group_w=None, group_rows=0):
    """Chan merge of forward partials [2][N][blocks] -> (count, mean [N], M2 [N]) of the expanded
    batch: what ured_bn_fwd_finalize / ured_bn_stats compute in fp64 before normalising. Also
    returns (sum |count_b * mean_b|) / count, the size of the terms the mean is a sum of."""
    ws = f64(ws)
    cnt, w = block_counts(M, group_w, group_rows)
    Mw = cnt.sum()
    mean = (ws[0] * cnt).sum(1) / Mw
    m2 = (ws[1] * w + cnt * (ws[0] - mean[:, None]) ** 2).sum(1)
    return Mw, mean, m2, (ws[0].abs() * cnt).sum(1) / Mw


def bn_outputs(Mw, mean, m2, eps=1e-5, momentum=0.1, rm=None, rv=None, gamma=None, beta=None):
    """mean, invstd (biased variance), scale, shift and the updated running statistics (unbiased
    variance; a single row keeps M2 as it is) from the merged (count, mean, M2)."""
    N = mean.shape[0]
    gamma = torch.ones(N, dtype=torch.float64) if gamma is None else f64(gamma)
    beta = torch.zeros(N, dtype=torch.float64) if beta is None else f64(beta)
    invstd = 1.0 / torch.sqrt(m2 / Mw + eps)
    scale = gamma * invstd
    out = {"count": Mw, "mean": mean, "m2": m2, "invstd": invstd, "scale": scale, "shift": beta - mean * scale,
           "var_unbiased": m2 / (Mw - 1.0) if Mw > 1 else m2}
    if rm is not None:
        out["running_mean"] = (1.0 - momentum) * f64(rm) + momentum * mean
    if rv is not None:
        out["running_var"] = (1.0 - momentum) * f64(rv) + momentum * out["var_unbiased"]
    return out


def bn_train_stats(p, w_rows=None, eps=1e-5, momentum=0.1, rm=None, rv=None, gamma=None, beta=None):
    """Training-mode BatchNorm statistics of the batch in which stored row r occurs w_rows[r] times."""
    p = f64(p)
    w = torch.ones(p.shape[0], dtype=torch.float64) if w_rows is None else f64(w_rows)
    Mw = w.sum()
    mean = (w[:, None] * p).sum(0) / Mw
    m2 = (w[:, None] * (p - mean) ** 2).sum(0)
    return bn_outputs(Mw, mean, m2, eps, momentum, rm, rv, gamma, beta)


def bn_coefs(dbeta, dgamma, Mw, invstd, gamma=None):
    """The ured_bn_bwd_apply coefficients: dP = a*g + w*(b*(p - mean) + c)."""
    invstd = f64(invstd)
    k = invstd if gamma is None else f64(gamma) * invstd
    return k, -k * invstd * dgamma / Mw, -k * dbeta / Mw


def bwd_finalize_terms(ws, M, gamma, invstd, group_w=None, group_rows=0):
    """ured_bn_bwd_finalize in float64 from backward partials [2][N][blocks]: -> (values, sizes),
    two dicts over dbeta / dgamma / ca / cb / cc; a size is the value's formula with the partials
    replaced by their magnitudes (what a rounding bound has to be relative to when the sums cancel)."""
    w = f64(ws)
    cnt, _ = block_counts(M, group_w, group_rows)
    Mw = cnt.sum()
    db, dg, adb, adg = w[0].sum(1), w[1].sum(1), w[0].abs().sum(1), w[1].abs().sum(1)
    a, b, c = bn_coefs(db, dg, Mw, invstd, gamma)
    k = a.abs()
    val = {"dbeta": db, "dgamma": dg, "ca": a, "cb": b, "cc": c, "count": Mw}
    mag = {"dbeta": adb, "dgamma": adg, "ca": k, "cb": k * f64(invstd).abs() * adg / Mw, "cc": k * adb / Mw}
    return val, mag


def fwd_output_sizes(out, mean_terms, momentum, rm=None, rv=None, gamma=None, beta=None):
    """Sizes of the terms each ured_bn_fwd_finalize output is a sum of (`out` from bn_outputs)."""
    N = out["mean"].shape[0]
    be = torch.zeros(N, dtype=torch.float64) if beta is None else f64(beta).abs()
    mag = {"mean": mean_terms, "invstd": out["invstd"].abs(), "scale": out["scale"].abs(),
           "shift": be + mean_terms * out["scale"].abs()}
    if rm is not None:
        mag["running_mean"] = (1.0 - momentum) * f64(rm).abs() + momentum * mean_terms
    if rv is not None:
        mag["running_var"] = (1.0 - momentum) * f64(rv).abs() + momentum * out["var_unbiased"].abs()
    return mag


def bn_bwd(g_sum, p, mean, invstd, gamma=None, w_rows=None):
    """BatchNorm backward on stored rows: g_sum [M][N] is the gradient w.r.t. the BN output summed
    over each stored row's copies, p the BN input. -> dgamma, dbeta, dP (summed over the copies)
    = a*g_sum + w*(b*(p - mean) + c), with the weighted row count in b and c."""
    g, p, mean, invstd = f64(g_sum), f64(p), f64(mean), f64(invstd)
    w = torch.ones(p.shape[0], dtype=torch.float64) if w_rows is None else f64(w_rows)
    xhat = (p - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    a, b, c = bn_coefs(dbeta, dgamma, w.sum(), invstd, gamma)
    return dgamma, dbeta, a * g + w[:, None] * (b * (p - mean) + c)


def act_terms(dh_sum, y, act, mean, invstd, scale=None, shift=None):
    """g (gradient at the BN output), p (BN input) and xhat of one layer for an activation order."""
    dh, y, mean, invstd = f64(dh_sum), f64(y), f64(mean), f64(invstd)
    if act == ACT_ENC:
        g = torch.where(y * f64(scale) + f64(shift) > 0, dh, torch.zeros_like(dh))
        p = y
    elif act == ACT_RES:
        g, p = dh, y.clamp_min(0)
    else:
        g, p = dh, y
    return g, p, (p - mean) * invstd


def bn_bwd_act(dh_sum, y, act, mean, invstd, scale=None, shift=None, gamma=None, w_rows=None):
    """Backward of one Conv+BN(+ReLU) layer down to dY, the gradient of the conv output y."""
    g, p, xhat = act_terms(dh_sum, y, act, mean, invstd, scale, shift)
    dgamma, dbeta, dp = bn_bwd(g, p, mean, invstd, gamma, w_rows)
    if act == ACT_RES:
        dp = torch.where(f64(y) > 0, dp, torch.zeros_like(dp))
    return {"g": g, "p": p, "xhat": xhat, "dgamma": dgamma, "dbeta": dbeta, "dY": dp}


def pool_ref(Y32, group_rows, scale, shift, relu):
    """Max-pool of act(scale*Y+shift) over groups of group_rows rows of the STORED fp32 Y: the
    winner is the argmax of Y where scale >= 0 and the argmin where scale < 0, lowest row on ties
    (global row index). -> pooled float64 [G][N], argidx int64 [G][N], the winning Y values."""
    Y = f64(Y32)
    M, N = Y.shape
    G = M // group_rows
    sc, sh = f64(scale), f64(shift)
    Yg = Y[:G * group_rows].view(G, group_rows, N)
    signed = torch.where(sc >= 0, Yg, -Yg)
    best = signed.max(1, keepdim=True).values
    rows = torch.arange(group_rows).view(1, group_rows, 1).expand(G, group_rows, N)
    first = torch.where(signed == best, rows, torch.full_like(rows, group_rows)).min(1).values
    by = Yg.gather(1, first.unsqueeze(1)).squeeze(1)
    pooled = by * sc + sh
    if relu:
        pooled = pooled.clamp_min(0)
    return pooled, first + torch.arange(G).view(G, 1) * group_rows, by


def ulp32(x):
    """Spacing of fp32 at |x| (float64 tensor in, float64 out; the normal range)."""
    x = f64(x).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)
