"""Float64 restatements of the loss-head entry points (csrc/loss.hip; contracts in
include/ured_hip.h), one function per entry point with the entry point's own inputs, shared by
tests/test_loss_kernels_gpu.py. Plain torch / numpy on the CPU. tests/test_loss_ref.py pins this
module to the oracle's loss functions (oracle/ured_ref.py: compute_cm_loss, contrast_loss,
residual_retrieval_loss, pc_consistency[_weighted]) and to torch autograd, so the GPU tests compare
kernels with arithmetic that has an independent check of its own.

Layout (include/ured_hip.h): half-sample s = h * B + b (h = 0 the deformed shape, 1 its mirror
image); k int64 [B] parts per sample; counts int64 [B, P]; off int32 [B*P + 1], off[b*P + i] the
first row of part i of sample b among the B*N sorted rows; gid int32 [B*N] the part slot b*P + i of
each sorted row. What the header leaves open and the kernels fix:
  * a part slot i >= k_b gets the segment (s*S + i*NP, 0, off[b*P + i] + h*B*N, 0): both lengths 0,
    the offsets those of a valid slot;
  * a valid part with counts == 0 contributes a_i / NP and nothing from the empty side;
  * k_b == 0 makes both of the sample's terms nan.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ured_ref

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
LT = 256                    # threads per workgroup of the reduction kernels


def f64(t, dtype=torch.float64):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", dtype)


def _ints(t):
    return torch.as_tensor(t).detach().cpu().long()


# ---------------------------------------------------------------------------------------------
# chamfer pair
# ---------------------------------------------------------------------------------------------
def parts_table(counts, N):
    """counts int64 [B,P] (every row sums to N) -> (off int32 [B*P + 1], gid int32 [B*N]) of sorted
    rows that hold part 0's points first, then part 1's, ...; a slot without points starts where
    the previous one ends."""
    counts = _ints(counts)
    B, P = counts.shape
    assert (counts.sum(1) == N).all() and (counts >= 0).all()
    start = torch.cumsum(counts, 1) - counts + N * torch.arange(B).unsqueeze(1)
    off = torch.cat([start.reshape(-1), torch.tensor([B * N])]).int()
    slot = (torch.arange(B * P)).repeat_interleave(counts.reshape(-1))
    return off, slot.int()


def cd_prep(out, x, x_sorted, k, counts, off, B, S, N, P, NP):
    """-> A [2B,S,3], X2, XS2 [2B,N,3] (the inputs' dtype: copies and one sign flip, so exact) and
    the int32 segment tables segs_full [2B,4], segs_part [2B*P,4] of (a_off, a_len, b_off, b_len)."""
    out, x, xs = (torch.as_tensor(v).detach().cpu() for v in (out, x, x_sorted))
    k, counts, off = _ints(k), _ints(counts).reshape(B, P), _ints(off)
    A = torch.cat([out, ured_ref.get_symmetric(out)]).reshape(2 * B, S, 3)
    X2 = torch.cat([x, x]).reshape(2 * B, N, 3)
    XS2 = torch.cat([xs, xs]).reshape(2 * B, N, 3)
    segf = torch.empty(2 * B, 4, dtype=torch.int32)
    segp = torch.empty(2 * B * P, 4, dtype=torch.int32)
    for s in range(2 * B):
        h, b = divmod(s, B)
        kb = int(k[b])
        segf[s] = torch.tensor([s * S, kb * NP, s * N, N], dtype=torch.int32)
        for i in range(P):
            v = i < kb
            segp[s * P + i] = torch.tensor([s * S + i * NP, NP if v else 0, int(off[b * P + i]) + h * B * N,
                                            int(counts[b, i]) if v else 0], dtype=torch.int32)
    return A, X2, XS2, segf, segp


def cd_reduce(daf, dbf, dap, dbp, k, counts, off, B, S, N, P, NP):
    """The four scalars [full, part, mirror full, mirror part] (float64 [4]) from the NN distances
    of the two families (dist_a_* [2B*S], dist_b_* [2B*N]):
      full_s = sum_a / (k_b NP) + sum_b / N,  part_s = (1/k_b) sum_{i<k_b} (a_i / NP + b_i / cnt_i),
    means over B of each half. Also the longest run of one fp32 block sum (for the rounding bound)."""
    daf, dbf, dap, dbp = (f64(v).reshape(-1) for v in (daf, dbf, dap, dbp))
    k, counts, off = _ints(k), _ints(counts).reshape(B, P), _ints(off)
    terms = torch.zeros(4, dtype=torch.float64)
    longest = max(N, NP)
    for s in range(2 * B):
        h, b = divmod(s, B)
        kb = int(k[b])
        if kb == 0:
            terms[2 * h:2 * h + 2] = float("nan")
            continue
        full = daf[s * S:s * S + kb * NP].sum() / (kb * NP) + dbf[s * N:(s + 1) * N].sum() / N
        part = torch.zeros((), dtype=torch.float64)
        for i in range(kb):
            a0 = s * S + i * NP
            part = part + dap[a0:a0 + NP].sum() / NP
            cnt = int(counts[b, i])
            if cnt > 0:
                b0 = int(off[b * P + i]) + h * B * N
                part = part + dbp[b0:b0 + cnt].sum() / cnt
                longest = max(longest, cnt)
        terms[2 * h] += full / B
        terms[2 * h + 1] += part / kb / B
    return terms, longest


def cd_grad(g4, k, counts, gid, B, S, N, P, NP):
    """Upstream weights of every NN distance, float64: (gd_a_full [2BS], gd_b_full [2BN], gd_a_part
    [2BS], gd_b_part [2BN]) and the zeroed accumulator ga [2BS, 3]."""
    g4, k, counts, gid = f64(g4), _ints(k), _ints(counts).reshape(B, P), _ints(gid)
    gaf, gap = torch.zeros(2 * B, S, dtype=torch.float64), torch.zeros(2 * B, S, dtype=torch.float64)
    gbf, gbp = torch.zeros(2 * B, N, dtype=torch.float64), torch.zeros(2 * B, N, dtype=torch.float64)
    for s in range(2 * B):
        h, b = divmod(s, B)
        kb = int(k[b])
        gbf[s] = g4[2 * h] / (B * N)
        if kb == 0:
            continue
        gaf[s, :kb * NP] = g4[2 * h] / (B * kb * NP)
        gap[s, :kb * NP] = g4[2 * h + 1] / (B * kb * NP)
        i = gid[b * N:(b + 1) * N] % P
        cnt = counts[b][i]
        on = (i < kb) & (cnt > 0)
        gbp[s] = torch.where(on, g4[2 * h + 1] / (B * kb * cnt.clamp_min(1).double()), torch.zeros((), dtype=torch.float64))
    return gaf.reshape(-1), gbf.reshape(-1), gap.reshape(-1), gbp.reshape(-1), torch.zeros(2 * B * S, 3, dtype=torch.float64)


def cd_fold(ga, B, S):
    """g [B,S,3] = ga[:B] + mirror(ga[B:]) (the mirror image's gradient folded back), ga's dtype."""
    ga = torch.as_tensor(ga).detach().cpu().reshape(2, B, S, 3)
    return ga[0] + ured_ref.get_symmetric(ga[1])


# ---------------------------------------------------------------------------------------------
# residual + reconstruction losses
# ---------------------------------------------------------------------------------------------
def point_losses(x, out, knn, res, rec, recu, ptsu, inv, mask, g4=None):
    """terms float64 [4] (res L1, res reg, recon full, recon src) on the GIVEN x -> out neighbour
    indices knn [B,N] (within the sample's rows); with g4 [4] also (dres, drec, drecu) of
    sum_i g4_i term_i by float64 autograd. recu None / U == 0: term 3 is nan and drecu None."""
    x, out = f64(x), f64(out)
    B, N, _ = x.shape
    res, rec = f64(res).requires_grad_(True), f64(rec).requires_grad_(True)
    nn = out[torch.arange(B).unsqueeze(1), _ints(knn).reshape(B, N)]
    t0 = (x + res - nn).abs().sum(-1).mean()
    t1 = res.abs().sum(-1).mean()
    t2 = ured_ref.pc_consistency(rec, x)
    U = 0 if recu is None else recu.shape[0]
    if U:
        recu = f64(recu).requires_grad_(True)
        inv = _ints(inv)
        R, NP = inv.shape[0], recu.shape[1]
        t3 = ured_ref.pc_consistency_weighted(recu[inv].view(1, R, NP, 3), f64(ptsu)[inv].view(1, R, NP, 3),
                                              f64(mask).view(1, R))
    else:
        t3 = torch.tensor(float("nan"), dtype=torch.float64)
    terms = torch.stack([t0, t1, t2, t3]).detach()
    if g4 is None:
        return terms
    g4 = f64(g4)
    (g4[0] * t0 + g4[1] * t1 + g4[2] * t2).backward()
    if U:
        (g4[3] * t3).backward()
    return terms, res.grad, rec.grad, (recu.grad if U else None)


# ---------------------------------------------------------------------------------------------
# contrastive loss
# ---------------------------------------------------------------------------------------------
def contrast(t, s_all, src_labels, s_off, scale, g=1.0, dtype=torch.float64):
    """-> dict(loss, dt [n,C], ds [n,C], inv [n + n_all], lse [n]) in float64: CE(scale * norm(t)
    norm(s_all)^T) with labels s_off + i (-1 where src_labels is -1, ignored), times the upstream g
    for the gradients. ds is the gradient of this rank's rows s_all[s_off : s_off + n] only.
    dtype = torch.float32 gives the same composition of torch ops in fp32 (a yardstick for what
    fp32 arithmetic costs on these inputs, not a reference)."""
    t = f64(t, dtype).requires_grad_(True)
    s_all = f64(s_all, dtype)
    n = t.shape[0]
    s_loc = s_all[s_off:s_off + n].clone().requires_grad_(True)
    s_cat = torch.cat([s_all[:s_off], s_loc, s_all[s_off + n:]])
    labels = s_off + torch.arange(n)
    labels[_ints(src_labels).reshape(-1) == -1] = -1
    logits = float(scale) * F.normalize(t, dim=-1, p=2) @ F.normalize(s_cat, dim=-1, p=2).t()
    loss = F.cross_entropy(logits, labels, ignore_index=-1)
    (loss * float(g)).backward()
    inv = 1.0 / torch.cat([t.detach().norm(dim=-1), s_all.norm(dim=-1)]).clamp_min(1e-12)
    return dict(loss=loss.detach(), dt=t.grad, ds=s_loc.grad, inv=inv, lse=torch.logsumexp(logits.detach(), dim=1))


# ---------------------------------------------------------------------------------------------
# loss assembly
# ---------------------------------------------------------------------------------------------
def assemble(terms, weights, g=1.0):
    """The fp32 left-to-right sum s = s + term_i * w_i (np.float32 arithmetic: every product and
    sum rounded once, as the kernel's) and gterms_i = w_i * g. -> (np.float32, float32 array)."""
    s = np.float32(0.0)
    for t, w in zip(terms, weights):
        s = np.float32(s + np.float32(np.float32(t) * np.float32(w)))
    return s, (np.asarray(weights, np.float32) * np.float32(g)).astype(np.float32)
