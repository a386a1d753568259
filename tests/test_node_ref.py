"""tests/node_ref.py (the float64 restatement the graph-node kernel tests compare with) pinned on
the CPU to independent torch compositions, to 1e-12 relative of each result's largest element:
the GEMM to cat / F.linear / where, the BatchNorm to torch.nn.BatchNorm1d in double called once per
set with autograd, two-rank merged statistics and sums to the full set, the attention to autograd
through attention_graph.attention.softmax_attention on the channel-first view."""
import pytest
import torch

import node_ref as NR

RTOL = 1e-12


def _close(a, b, what=""):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel() == 0:
        return
    err, big = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= RTOL * big, (what, err, big)


def _rand(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("M,N,K,k1,n1", [(33, 70, 45, 16, 20), (1, 1, 1, None, None), (5, 7, 32, 0, None),
                                         (65, 31, 48, 48, 31), (4, 6, 0, None, None)])
def test_gemm_matches_direct_composition(M, N, K, k1, n1):
    g = torch.Generator().manual_seed(M + N + K)
    A, Bm = _rand(g, M, K), _rand(g, K, N)
    bias, rb, R, C0 = _rand(g, N), _rand(g, (M + 4) // 5, N), _rand(g, M, N), _rand(g, M, N)
    gate = _rand(g, M, N)
    gate[::3] = 0.0
    kw = {}
    if k1 is not None:
        kw.update(A2=A[:, k1:])
    if n1 is not None:
        kw.update(B2=Bm[:, n1:])
    a1 = None if k1 == 0 else (A if k1 is None else A[:, :k1])
    b1 = Bm if n1 is None else Bm[:, :n1]
    acc = torch.nn.functional.linear(A, Bm.t())
    _close(NR.gemm(a1, b1, **kw), acc, "plain")
    _close(NR.gemm(a1, b1, bias=bias, **kw), acc + bias, "bias")
    rbx = rb.repeat_interleave(5, 0)[:M]
    _close(NR.gemm(a1, b1, rowbias=rb, rdiv=5, **kw), acc + rbx, "rowbias")
    _close(NR.gemm(a1, b1, relu=True, **kw), torch.relu(acc), "relu")
    _close(NR.gemm(a1, b1, gate=gate, **kw), acc * (gate > 0), "gate")
    for nc in (N, N // 2, 0):
        Rp = torch.cat([R[:, :nc], torch.zeros(M, N - nc, dtype=torch.float64)], 1)
        _close(NR.gemm(a1, b1, R=R, R_ncols=nc, **kw), acc + Rp, f"R {nc}")
    _close(NR.gemm(a1, b1, C_old=C0, **kw), acc + C0, "accumulate")
    # all together, in the kernel's order: ReLU before the gate, residual and accumulation after both
    full = torch.relu(acc + bias + rbx) * (gate > 0) + torch.cat([R[:, :N // 2], torch.zeros(M, N - N // 2, dtype=torch.float64)], 1) + C0
    _close(NR.gemm(a1, b1, bias=bias, rowbias=rb, rdiv=5, relu=True, gate=gate, R=R, R_ncols=N // 2, C_old=C0, **kw),
           full, "all")
    # the order matters on this data: gate-then-ReLU equals it, but a residual inside the ReLU does not
    if M * N > 20:
        assert not torch.equal(full, torch.relu(acc + bias + rbx + R) * (gate > 0) + C0)


def test_colsum():
    g = torch.Generator().manual_seed(1)
    x, c = _rand(g, 17, 5), _rand(g, 5)
    want = torch.stack([x[:, j].sum() for j in range(5)])
    _close(NR.colsum(x), want)
    _close(NR.colsum(x, c, True), want + c)
    assert torch.equal(NR.colsum(x[:0]), torch.zeros(5, dtype=torch.float64))
    assert torch.equal(NR.colsum(x[:0], c, True), c)


@pytest.mark.parametrize("off", [(0, 2), (0, 63, 127), (0, 5, 70, 72, 137)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu_in", [True, False])
def test_bn_sets_match_batchnorm1d(off, training, relu_in):
    """Two consecutive calls, so that the running statistics and num_batches_tracked compound."""
    g = torch.Generator().manual_seed(len(off) + 2 * training + relu_in)
    N, R = 5, off[-1]
    bnm = torch.nn.BatchNorm1d(N, momentum=0.3, eps=1e-3).double().train(training)
    with torch.no_grad():
        bnm.weight.copy_(_rand(g, N))               # both signs
        bnm.bias.copy_(_rand(g, N))
        bnm.running_mean.copy_(_rand(g, N) * 0.1)
        bnm.running_var.copy_(torch.rand(N, generator=g, dtype=torch.float64) + 0.5)
    state = (bnm.running_mean.clone(), bnm.running_var.clone(), 0)
    gamma, beta = bnm.weight.detach().clone(), bnm.bias.detach().clone()
    for call in range(2):
        Y = _rand(g, R, N).requires_grad_(True)
        G = _rand(g, R, N)
        x = torch.relu(Y) if relu_in else Y
        act = torch.cat([bnm(x[a:b]) for a, b in zip(off[:-1], off[1:])])
        bnm.zero_grad()
        act.backward(G)
        r = NR.bn_sets(Y, off, gamma, beta, state[0], state[1], 0.3, 1e-3, training, relu_in, state[2])
        _close(r["act"], act.detach(), "act")
        _close(r["running_mean"], bnm.running_mean, "running_mean")
        _close(r["running_var"], bnm.running_var, "running_var")
        assert r["num_batches_tracked"] == int(bnm.num_batches_tracked) == (call + 1) * (len(off) - 1) * training
        if not training:
            assert torch.equal(r["running_mean"], state[0]) and torch.equal(r["running_var"], state[1])
        dY, dgamma, dbeta = NR.bn_sets_bwd(G, Y, off, gamma, r["mean"], r["invstd"], training, relu_in)
        _close(dY, Y.grad, "dY")
        _close(dgamma, bnm.weight.grad, "dgamma")
        _close(dbeta, bnm.bias.grad, "dbeta")
        state = (r["running_mean"], r["running_var"], r["num_batches_tracked"])


@pytest.mark.parametrize("relu_in", [True, False])
@pytest.mark.parametrize("split", [(5, 60), (1, 1), (64, 1)])
def test_two_rank_merge_equals_full_set(relu_in, split):
    g = torch.Generator().manual_seed(sum(split))
    N, R = 4, sum(split)
    Y, G = _rand(g, R, N) + 0.5, _rand(g, R, N)
    gamma, beta = _rand(g, N), _rand(g, N)
    rm, rv = _rand(g, N) * 0.1, torch.rand(N, generator=g, dtype=torch.float64) + 0.5
    full = NR.bn_sets(Y, (0, R), gamma, beta, rm, rv, 0.1, 1e-5, True, relu_in)
    a, b = Y[:split[0]], Y[split[0]:]
    merged = NR.merge_stats(NR.bn_rank_stats(a, relu_in), NR.bn_rank_stats(b, relu_in))
    whole = NR.bn_rank_stats(Y, relu_in)
    for i, what in enumerate(("count", "mean", "M2")):
        _close(merged[i], whole[i], what)
    mean, invstd, unb = NR.stats_to_bn(merged, 1e-5)
    _close(mean, full["mean"][0], "mean")
    _close(invstd, full["invstd"][0], "invstd")
    _close(0.9 * rv + 0.1 * unb, full["running_var"], "running_var")
    _close(0.9 * rm + 0.1 * mean, full["running_mean"], "running_mean")
    # backward: the ranks' sums add up to the set's, and each rank's dY rows follow from the total
    sums = NR.bn_rank_sums(G[:split[0]], a, mean, invstd, relu_in) + NR.bn_rank_sums(G[split[0]:], b, mean, invstd, relu_in)
    dY, dgamma, dbeta = NR.bn_sets_bwd(G, Y, (0, R), gamma, full["mean"], full["invstd"], True, relu_in)
    _close(sums[0], dbeta, "sum g")
    _close(sums[1], dgamma, "sum g xhat")
    assert torch.equal(sums[2], torch.full((N,), float(R), dtype=torch.float64))
    x = Y.clamp(min=0) if relu_in else Y
    dx = gamma * invstd * (G - sums[0] / sums[2] - (x - mean) * invstd * sums[1] / sums[2])
    _close(torch.where(Y > 0, dx, torch.zeros_like(dx)) if relu_in else dx, dY, "dY from the merged sums")


@pytest.mark.parametrize("B,H,n,m,d,mul", [(2, 2, 5, 7, 16, 1.0), (1, 1, 1, 1, 1, 1.0), (3, 3, 7, 1, 5, 1.0),
                                           (2, 2, 5, 7, 16, 12.0), (1, 2, 32, 32, 8, 6.0)])
def test_attention_matches_softmax_attention_autograd(B, H, n, m, d, mul):
    from attention_graph.attention import softmax_attention
    g = torch.Generator().manual_seed(n * 31 + m + d)
    C = H * d
    q, k, v = _rand(g, B, n, C) * mul, _rand(g, B, m, C) * mul, _rand(g, B, m, C)
    go = _rand(g, B, n, C)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    cf = [t.permute(0, 2, 1).reshape(B, H, d, t.shape[1]) for t in leaves]      # the reference's view(B, H, d, n)
    out_cf, w = softmax_attention(*cf)
    out_ref = out_cf.reshape(B, C, n).permute(0, 2, 1)
    out_ref.backward(go)
    out, P = NR.attn_fwd(q, k, v, H, d ** -0.5)
    _close(out, out_ref.detach(), "out")
    _close(P, w.detach(), "weights")
    for got, leaf, what in zip(NR.attn_bwd(q, k, v, P, go, H, d ** -0.5), leaves, ("dq", "dk", "dv")):
        _close(got, leaf.grad, what)
