"""tests/loss_ref.py (the float64 restatements the loss-head kernel tests compare with) against
something independent: the oracle's loss functions (oracle/ured_ref.py, each pinned to the
reference by tests/test_oracle_golden.py), the C nearest-neighbour oracle and torch autograd.
Float64 against float64 agrees to 1e-12 relative; where the other side is the oracle's fp32 NN
backward the comparison is at 2e-6 of the largest entry. Runs on the CPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref
from oracle import nn_ref, ured_ref

RTOL = 1e-12


def _close(got, ref, name, rtol=RTOL):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    scale = max(ref.abs().max().item(), 1e-300)
    err = (got - ref).abs().max().item()
    assert err <= rtol * scale, f"{name}: {err:.3e} > {rtol:.0e} * {scale:.3e}"


def _cd_case(seed=0):
    """B = 2, P = 3, S > P*NP, k = (3, 2), every valid part non-empty; x_sorted = x permuted."""
    g = torch.Generator().manual_seed(seed)
    B, P, NP, N = 2, 3, 5, 11
    S = P * NP + 2
    out = torch.randn(B, S, 3, generator=g)
    x = torch.randn(B, N, 3, generator=g)
    xs = torch.stack([x[b][torch.randperm(N, generator=g)] for b in range(B)])
    k = torch.tensor([3, 2])
    counts = torch.tensor([[4, 3, 4], [5, 6, 0]])
    off, gid = loss_ref.parts_table(counts, N)
    return dict(B=B, P=P, NP=NP, N=N, S=S, out=out, x=x, xs=xs, k=k, counts=counts, off=off, gid=gid)


def _oracle_cm(c, out64):
    B, P = c["B"], c["P"]
    part_x = [[c["xs"][b, int(c["off"][b * P + i]) - b * c["N"]:][:int(c["counts"][b, i])].double()
               for i in range(int(c["k"][b]))] for b in range(B)]
    mask = (torch.arange(P).unsqueeze(0) < c["k"].unsqueeze(1)).double()
    x64 = c["x"].double()
    return (*ured_ref.compute_cm_loss(out64, x64, part_x, mask, np_per_part=c["NP"]),
            *ured_ref.compute_cm_loss(ured_ref.get_symmetric(out64), x64, part_x, mask, np_per_part=c["NP"]))


def _families(c):
    dims = (c["B"], c["S"], c["N"], c["P"], c["NP"])
    A, X2, XS2, segf, segp = loss_ref.cd_prep(c["out"], c["x"], c["xs"], c["k"], c["counts"], c["off"], *dims)
    full = nn_ref.nn_seg_fwd(A.numpy(), X2.numpy(), segf.numpy())
    part = nn_ref.nn_seg_fwd(A.numpy(), XS2.numpy(), segp.numpy())
    return dims, A, X2, XS2, segf, segp, full, part


def test_cd_prep_reduce_reproduce_compute_cm_loss():
    c = _cd_case()
    dims, A, X2, XS2, segf, segp, full, part = _families(c)
    assert torch.equal(A[c["B"]:], ured_ref.get_symmetric(c["out"])) and torch.equal(X2[:c["B"]], X2[c["B"]:])
    terms, longest = loss_ref.cd_reduce(full[0], full[2], part[0], part[2], c["k"], c["counts"], c["off"], *dims)
    want = torch.stack(_oracle_cm(c, c["out"].double()))
    _close(terms, want, "cd terms")
    assert longest == c["N"]


def _nn_bwd64(A, Bp, segs, gd_a, gd_b, ia, ib, ga):
    """a-side NN backward in float64: d sum(gd_a * dist_a + gd_b * dist_b) / d A, added to ga."""
    for ao, al, bo, bl in segs.tolist():
        for i in range(al):
            ga[ao + i] += 2 * gd_a[ao + i] * (A[ao + i] - Bp[bo + int(ia[ao + i])])
        for j in range(bl):
            q = ao + int(ib[bo + j])
            ga[q] += 2 * gd_b[bo + j] * (A[q] - Bp[bo + j])


def test_cd_grad_fold_reproduce_autograd():
    c = _cd_case(1)
    dims, A, X2, XS2, segf, segp, full, part = _families(c)
    B, S = c["B"], c["S"]
    g4 = torch.tensor([0.7, -1.3, 2.0, 0.4], dtype=torch.float64)
    gaf, gbf, gap, gbp, ga = loss_ref.cd_grad(g4, c["k"], c["counts"], c["gid"], *dims)
    assert ga.shape == (2 * B * S, 3) and not ga.any()
    # the weights are the loss's derivative by every distance: the terms are linear in them
    terms, _ = loss_ref.cd_reduce(full[0], full[2], part[0], part[2], c["k"], c["counts"], c["off"], *dims)
    lin = sum((w * loss_ref.f64(d)).sum() for w, d in ((gaf, full[0]), (gbf, full[2]), (gap, part[0]), (gbp, part[2])))
    _close(lin, (g4 * terms).sum(), "sum of weights * distances")
    A64 = A.double().reshape(-1, 3)
    _nn_bwd64(A64, X2.double().reshape(-1, 3), segf, gaf, gbf, full[1], full[3], ga)
    _nn_bwd64(A64, XS2.double().reshape(-1, 3), segp, gap, gbp, part[1], part[3], ga)
    got = loss_ref.cd_fold(ga, B, S)
    out64 = c["out"].double().requires_grad_(True)
    (g4 * torch.stack(_oracle_cm(c, out64))).sum().backward()
    _close(got, out64.grad, "d out", rtol=2e-6)       # the oracle's NN backward is fp32
    fold32 = loss_ref.cd_fold(ga.float(), B, S)
    assert fold32.dtype == torch.float32 and torch.equal(fold32[..., 0], ga.float().view(2, B, S, 3)[0, ..., 0]
                                                         - ga.float().view(2, B, S, 3)[1, ..., 0])


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 3), (2, 3)])
def test_contrast_reproduces_oracle(rank, world):
    g = torch.Generator().manual_seed(rank)
    B, Pn, C = 2, 3, 8
    n = B * Pn
    t = torch.randn(B, Pn, C, generator=g, dtype=torch.float64).requires_grad_(True)
    s = torch.randn(B, Pn, C, generator=g, dtype=torch.float64).requires_grad_(True)
    others = torch.randn(world * n, C, generator=g, dtype=torch.float64)
    src_labels = torch.tensor([[4, -1, 7], [0, 2, -1]])
    s_off = rank * n
    if world == 1:
        want = ured_ref.contrast_loss(t, s, src_labels)
        s_all = s.detach().reshape(n, C)
    else:
        s_all = others.clone()
        s_all[s_off:s_off + n] = s.detach().reshape(n, C)
        gathered = torch.cat([F.normalize(others[:s_off], dim=-1), F.normalize(s.reshape(n, C), dim=-1),
                              F.normalize(others[s_off + n:], dim=-1)])
        want = ured_ref.contrast_loss(t, s, src_labels, rank=rank, gathered_src=gathered)
    (want * -2.5).backward()
    scale = float(torch.tensor(math.log(1 / 0.07)).exp())
    got = loss_ref.contrast(t.detach().reshape(n, C), s_all, src_labels, s_off, scale, g=-2.5)
    _close(got["loss"], want.detach(), "loss")
    _close(got["dt"], t.grad.reshape(n, C), "dt")
    _close(got["ds"], s.grad.reshape(n, C), "ds")
    _close(got["inv"][:n], 1 / t.detach().reshape(n, C).norm(dim=-1), "inv")
    assert got["lse"].shape == (n,) and got["inv"].shape == (n + world * n,)


def test_point_losses_reproduce_oracle():
    g = torch.Generator().manual_seed(3)
    B, N, P, NP, U = 2, 40, 3, 6, 4
    S = P * NP
    x = torch.randn(B, N, 3, generator=g)
    out = torch.randn(B, S, 3, generator=g)
    res = torch.randn(B, N, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    rec = torch.randn(B, N, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    recu = torch.randn(U, NP, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    ptsu = torch.randn(U, NP, 3, generator=g, dtype=torch.float64)
    inv = torch.tensor([0, 2, 2, 3, 0, 2])                      # part 1 unused, part 2 three times
    mask = torch.tensor([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]], dtype=torch.float64)
    knn = torch.stack([torch.from_numpy(nn_ref.nn_dir(x[b].numpy(), out[b].numpy())[1]) for b in range(B)])
    x64 = x.double()
    t0, t1 = ured_ref.residual_retrieval_loss(x64, out.double(), res, torch.ones(B, P), np_per_part=NP)
    t2 = ured_ref.pc_consistency(rec, x64)
    t3 = ured_ref.pc_consistency_weighted(recu[inv].view(B, P, NP, 3), ptsu[inv].view(B, P, NP, 3), mask)
    g4 = torch.tensor([1.5, -0.5, 2.0, -3.0], dtype=torch.float64)
    (g4 * torch.stack([t0, t1, t2, t3])).sum().backward()
    terms, dres, drec, drecu = loss_ref.point_losses(x, out, knn, res.detach(), rec.detach(), recu.detach(), ptsu, inv,
                                                     mask.reshape(-1), g4)
    _close(terms, torch.stack([t0, t1, t2, t3]).detach(), "terms")
    _close(dres, res.grad, "dres")
    _close(drec, rec.grad, "drec")
    _close(drecu, recu.grad, "drecu")
    assert not drecu[1].any() and drecu[2].any()
    # U == 0: three terms and two gradients as before, term 3 nan
    terms0, dres0, drec0, none = loss_ref.point_losses(x, out, knn, res.detach(), rec.detach(), None, None, None, None, g4)
    assert torch.equal(terms0[:3], terms[:3]) and math.isnan(terms0[3]) and none is None
    assert torch.equal(dres0, dres) and torch.equal(drec0, drec)


def test_assemble_is_the_fp32_left_to_right_sum():
    terms = [0.1, 1e8, -1e8, 3.0]
    w = [1.0, 1.0, 1.0, 0.5]
    s, gt = loss_ref.assemble(terms, w, g=-2.0)
    assert s == np.float32(1.5) and s.dtype == np.float32          # 0.1 is lost against 1e8, as in fp32
    assert gt.dtype == np.float32 and gt.tolist() == [-2.0, -2.0, -2.0, -1.0]
    assert loss_ref.assemble([0.1, 0.2], [3.0, 7.0])[0] == np.float32(np.float32(np.float32(0.1) * np.float32(3.0))
                                                                      + np.float32(0.2) * np.float32(7.0))


def test_torch_behaviours_the_gpu_tests_rely_on():
    """All rows ignored: loss nan and zero gradients. A zero row (norm clamped to 1e-12): finite
    gradients of order 1e12, d x = d xhat / eps with no projection term."""
    g = torch.Generator().manual_seed(5)
    t = torch.randn(4, 8, generator=g, dtype=torch.float64)
    s = torch.randn(4, 8, generator=g, dtype=torch.float64)
    r = loss_ref.contrast(t, s, torch.full((4,), -1), 0, 14.0)
    assert math.isnan(r["loss"]) and not r["dt"].any() and not r["ds"].any()
    t[1] = 0
    s[2] = 0
    r = loss_ref.contrast(t, s, torch.zeros(4, dtype=torch.long), 0, 14.0)
    assert math.isfinite(r["loss"]) and torch.isfinite(r["dt"]).all() and torch.isfinite(r["ds"]).all()
    assert 1e10 < r["dt"][1].abs().max() < 1e14 and 1e10 < r["ds"][2].abs().max() < 1e14
    assert r["inv"][1] == 1e12 and r["inv"][4 + 2] == 1e12
    # a nonzero row below the clamp: the gradient is d xhat / eps exactly (the clamp is a constant)
    t[1] = 1e-14
    r2 = loss_ref.contrast(t, s, torch.zeros(4, dtype=torch.long), 0, 14.0)
    th = (t[1] * 1e12).requires_grad_(True)
    sn = F.normalize(s, dim=-1)
    tn = torch.cat([F.normalize(t[:1], dim=-1), th.unsqueeze(0), F.normalize(t[2:], dim=-1)])
    F.cross_entropy(14.0 * tn @ sn.t(), torch.arange(4)).backward()
    _close(r2["dt"][1], th.grad * 1e12, "clamped row")
