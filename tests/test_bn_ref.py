"""tests/bn_ref.py (the float64 restatement the BN / pool kernel tests compare with) against
something independent: torch.nn.functional.batch_norm in float64 through autograd, on the batch
expanded with repeat_interleave. Each stored row's upstream gradient is split evenly over its
copies; running statistics, dgamma and dbeta must equal the helper's and the copies' input
gradients must sum to the helper's dY, all to 1e-12 relative. Runs on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref

RTOL = 1e-12


def _close(got, ref, name):
    scale = max(ref.abs().max().item(), 1e-300)
    err = (got - ref).abs().max().item()
    assert err <= RTOL * scale, f"{name}: {err:.3e} > {RTOL:.0e} * {scale:.3e}"


def _case(M, N, group_w, group_rows, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, N, generator=g, dtype=torch.float64) * 1.5 + 0.3
    dh = torch.randn(M, N, generator=g, dtype=torch.float64)
    gamma = torch.randn(N, generator=g, dtype=torch.float64)        # both signs
    beta = torch.randn(N, generator=g, dtype=torch.float64)
    rm = torch.randn(N, generator=g, dtype=torch.float64)
    rv = torch.rand(N, generator=g, dtype=torch.float64) + 0.5
    w_rows = bn_ref.row_weights(group_w, group_rows, M)
    return y, dh, gamma, beta, rm, rv, w_rows


# weights per group of group_rows rows; M = 10 is not a multiple of the group size 4
@pytest.mark.parametrize("group_w", [[1, 3, 2], [1, 1, 1], None], ids=["w132", "ones", "none"])
@pytest.mark.parametrize("act", [bn_ref.ACT_ENC, bn_ref.ACT_RES, bn_ref.ACT_BN], ids=["enc", "res", "bn"])
@pytest.mark.parametrize("M,group_rows", [(10, 4), (12, 4), (300, 128)])
def test_weighted_bn_matches_expanded_autograd(group_w, act, M, group_rows):
    N, eps, mom = 5, 1e-5, 0.1
    y, dh, gamma, beta, rm, rv, w_rows = _case(M, N, group_w, group_rows, 11 * M + act)
    reps = torch.ones(M, dtype=torch.long) if w_rows is None else w_rows.long()

    # independent path: the expanded batch through torch's batch_norm and autograd
    ye = y.repeat_interleave(reps, 0).requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    p = torch.relu(ye) if act == bn_ref.ACT_RES else ye
    out = F.batch_norm(p, rm_t, rv_t, ga, be, True, mom, eps)
    if act == bn_ref.ACT_ENC:
        out = torch.relu(out)
    up = (dh / reps[:, None].double()).repeat_interleave(reps, 0)      # split evenly over the copies
    out.backward(up)
    owner = torch.arange(M).repeat_interleave(reps)
    dy_sum = torch.zeros(M, N, dtype=torch.float64).index_add_(0, owner, ye.grad)

    # the helper, on stored rows only
    pst = y.clamp_min(0) if act == bn_ref.ACT_RES else y
    st = bn_ref.bn_train_stats(pst, w_rows, eps, mom, rm, rv, gamma, beta)
    _close(st["running_mean"], rm_t, "running_mean")
    _close(st["running_var"], rv_t, "running_var")
    assert st["count"].item() == float(reps.sum())
    bw = bn_ref.bn_bwd_act(dh, y, act, st["mean"], st["invstd"], st["scale"], st["shift"], gamma, w_rows)
    _close(bw["dgamma"], ga.grad, "dgamma")
    _close(bw["dbeta"], be.grad, "dbeta")
    _close(bw["dY"], dy_sum, "dY summed over copies")
    # the forward itself: act(scale*y+shift) is the module's output on every copy
    mine = pst * st["scale"] + st["shift"]
    if act == bn_ref.ACT_ENC:
        mine = mine.clamp_min(0)
    _close(mine.repeat_interleave(reps, 0), out.detach(), "forward")


@pytest.mark.parametrize("M", [1, 127, 129, 300])
@pytest.mark.parametrize("group_w,group_rows", [(None, 0), ([1, 3, 2], 128), ([1, 3, 2], 256)], ids=["none", "w128", "w256"])
def test_partials_merge_to_batch_stats(M, group_w, group_rows):
    """block_partials -> merge_partials (the Chan merge the finalize kernels restate) gives the
    statistics of the expanded rows; the backward partials sum to dbeta / dgamma."""
    g = torch.Generator().manual_seed(M)
    p = torch.randn(M, 3, generator=g, dtype=torch.float64) + 0.5
    w_rows = bn_ref.row_weights(group_w, group_rows, M)
    Mw, mean, m2, _ = bn_ref.merge_partials(bn_ref.block_partials(p), M, group_w, group_rows)
    st = bn_ref.bn_train_stats(p, w_rows)
    assert Mw.item() == st["count"].item()
    _close(mean, st["mean"], "mean")
    assert (m2 - st["m2"]).abs().max().item() <= 1e-12 * max(st["m2"].abs().max().item(), 1.0)
    if M == 1:      # one row: the unbiased variance keeps M2 (= 0), no division by zero
        assert torch.equal(st["var_unbiased"], st["m2"]) and st["m2"].abs().max().item() == 0.0
    gr = torch.randn(M, 3, generator=g, dtype=torch.float64)
    xh = (p - st["mean"]) * st["invstd"]
    bp = bn_ref.block_bwd_partials(gr, xh)
    dgamma, dbeta, _ = bn_ref.bn_bwd(gr, p, st["mean"], st["invstd"], None, w_rows)
    _close(bp[0].sum(1), dbeta, "dbeta from partials")
    _close(bp[1].sum(1), dgamma, "dgamma from partials")
    # the finalize restatement: coefficients from the partials = those of the row formulas
    gamma = torch.randn(3, generator=g, dtype=torch.float64)
    val, mag = bn_ref.bwd_finalize_terms(bp, M, gamma, st["invstd"], group_w, group_rows)
    a, b, c = bn_ref.bn_coefs(dbeta, dgamma, st["count"], st["invstd"], gamma)
    for key, ref in (("ca", a), ("cb", b), ("cc", c)):
        assert (val[key] - ref).abs().max().item() <= 1e-12 * mag[key].max().item(), key
        assert (mag[key] >= val[key].abs() * (1 - 1e-12)).all()


def test_pool_ref_ties_and_signs():
    Y = torch.tensor([[1.0, 1.0, 0.0, 2.0],
                      [3.0, -2.0, 0.0, 2.0],
                      [3.0, -2.0, -0.0, 1.0],
                      [0.0, 5.0, 0.0, 2.0]])
    scale = torch.tensor([2.0, -1.0, 0.0, -0.5])
    shift = torch.tensor([0.5, 1.0, 0.25, -3.0])
    pooled, idx, best = bn_ref.pool_ref(Y, 4, scale, shift, relu=True)
    assert idx.tolist() == [[1, 1, 0, 2]]               # lowest row on ties; argmin where scale < 0
    assert best.tolist() == [[3.0, -2.0, 0.0, 1.0]]
    assert pooled.tolist() == [[6.5, 3.0, 0.25, 0.0]]   # -3.5 clamped
    pooled, idx, _ = bn_ref.pool_ref(Y, 2, scale, shift, relu=False)
    assert idx.tolist() == [[1, 1, 0, 0], [2, 2, 2, 2]]
    assert pooled.tolist() == [[6.5, 3.0, 0.25, -4.0], [6.5, 3.0, 0.25, -3.5]]
