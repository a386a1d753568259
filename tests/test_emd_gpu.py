"""§8(f)4 auction EMD (csrc/emd.hip) vs the C restatement (oracle/emd_oracle.c): assignment and
dist bit-exact (same deterministic auction, same fp32/fp64 expressions); quality against the
exact optimal matching (scipy.optimize.linear_sum_assignment) and the reference's own
self-check (emd_module.py:93-105: sqrt(dist) re-derived from the assignment)."""
import numpy as np
import pytest
import torch

from oracle import emd_ref

pytestmark = pytest.mark.gpu


def _clouds(b, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=g), torch.rand(b, n, 3, generator=g)


def _later_step_share(asg, n):
    """Share of assignments to objects that the bid kernel reads in its second or a later LDS step
    (offset >= 256 inside the object's quarter of ceil(n / 4)): what a defect there would change."""
    a = asg[asg >= 0]
    return float((a % -(-n // 4) >= 256).mean()) if a.size else 0.0


# n <= 1024 is one LDS step of 256 objects per quarter. Beyond: 1025 / 1027 (n4 = 257: a second step
# with one object per quarter, quarter 3 short in step 0 and empty in step 1), 2048 (the benchmark's
# and calc_emd's shape), 2049 (three steps), 4100 (five). 5 and 3: quarter 3 starts past n / is
# empty. iters = 0: no round, assignment -1 everywhere and dist to point 0.
@pytest.mark.parametrize("b,n,eps,iters", [(2, 100, 0.05, 20), (3, 257, 0.005, 50), (1, 1024, 0.02, 40),
                                           (2, 8, 0.5, 1), (1, 1, 0.005, 3),
                                           (2, 1025, 0.005, 50), (1, 1027, 0.02, 40), (2, 2048, 0.005, 50),
                                           (1, 2049, 0.01, 30), (1, 4100, 0.005, 20), (3, 5, 0.1, 4),
                                           (2, 3, 0.1, 4), (2, 70, 0.05, 0)])
def test_emd_bitexact_vs_oracle(dev, b, n, eps, iters):
    from emd import emd
    x1, x2 = _clouds(b, n, n + iters)
    dist, asg = emd()(x1.to(dev), x2.to(dev), eps, iters)
    rd, ra = emd_ref.emd_fwd(x1.numpy(), x2.numpy(), eps, iters)
    print(f"emd n={n}: oracle share of assignments beyond the first LDS step {_later_step_share(ra, n):.4f}")
    if iters == 0:
        assert (ra == -1).all()
    np.testing.assert_array_equal(asg.cpu().numpy(), ra)
    np.testing.assert_array_equal(dist.cpu().numpy(), rd)


def test_emd_duplicates_deterministic(dev):
    """Exact value ties (duplicate points): lowest-index rules, run-to-run identical."""
    from emd import emd
    x1, x2 = _clouds(2, 300, 1)
    x2[:, 150:] = x2[:, :150]
    x1[:, 1::2] = x1[:, ::2]
    d1, a1 = emd()(x1.to(dev), x2.to(dev), 0.01, 30)
    d2, a2 = emd()(x1.to(dev), x2.to(dev), 0.01, 30)
    assert torch.equal(a1, a2) and torch.equal(d1, d2)
    rd, ra = emd_ref.emd_fwd(x1.numpy(), x2.numpy(), 0.01, 30)
    np.testing.assert_array_equal(a1.cpu().numpy(), ra)


def test_emd_duplicates_across_quarters_and_steps(dev):
    """The same at n = 1300 (quarters of 325: two LDS steps each): object k and its copy 650 + k lie
    two quarters apart, at one offset, so every best value is tied across the quarter merge, in the
    first LDS step for offsets below 256 and in the second above; bidders come in equal pairs. The
    lowest index wins throughout; assignment and dist equal the oracle's and repeat bit for bit."""
    from emd import emd
    x1, x2 = _clouds(2, 1300, 1)
    x2[:, 650:] = x2[:, :650]
    x1[:, 1::2] = x1[:, ::2]
    d1, a1 = emd()(x1.to(dev), x2.to(dev), 0.01, 30)
    d2, a2 = emd()(x1.to(dev), x2.to(dev), 0.01, 30)
    assert torch.equal(a1, a2) and torch.equal(d1, d2)
    rd, ra = emd_ref.emd_fwd(x1.numpy(), x2.numpy(), 0.01, 30)
    np.testing.assert_array_equal(a1.cpu().numpy(), ra)
    np.testing.assert_array_equal(d1.cpu().numpy(), rd)


def _quality(dev, n, eps, oracle_precondition):
    from scipy.optimize import linear_sum_assignment
    from emd import emd
    x1, x2 = _clouds(1, n, 8 if oracle_precondition else 7)
    if oracle_precondition:
        # the C oracle alone reaches a bijection with these inputs (0.753 above the optimum, bound
        # n * eps = 11.0): asserted, so that another seed cannot make the check below vacuous
        _, ra = emd_ref.emd_fwd(x1.numpy(), x2.numpy(), eps, 3000)
        assert len(np.unique(ra[0])) == n and ra.min() >= 0
    dist, asg = emd()(x1.to(dev), x2.to(dev), eps, 3000)
    a = asg[0].cpu().numpy()
    assert len(np.unique(a)) == n                      # a bijection
    c = np.sqrt(((x1[0].numpy()[:, None, :] - x2[0].numpy()[None]) ** 2).sum(-1))
    r, k = linear_sum_assignment(c)
    opt = c[r, k].sum()
    got = c[np.arange(n), a].sum()
    print(f"emd quality n={n}: cost {got:.4f}, optimum {opt:.4f}, excess {got - opt:.4f} (bound {n * eps:.3f})")
    assert opt - 1e-4 <= got <= opt + n * eps + 1e-4
    # emd_module.py test_emd's own check: the distances re-derived from the assignment
    re = ((x1[0] - x2[0][torch.from_numpy(a).long()]) ** 2).sum(-1)
    np.testing.assert_allclose(dist[0].cpu().numpy(), re.numpy(), rtol=1e-6, atol=1e-7)


def test_emd_quality_vs_exact_matching(dev):
    """With many rounds the auction reaches a bijection whose cost is within n*eps of the optimal
    assignment (auction eps-optimality, on the benefit 3 - |x1 - x2|)."""
    _quality(dev, 256, 0.002, False)


def test_emd_quality_vs_exact_matching_two_lds_steps(dev):
    """The same above 1024 points (n = 1100, quarters of 275: a second LDS step of 19 objects), at
    eps = 0.01 where 3000 rounds converge (n = 1280 would need 8000-20000)."""
    _quality(dev, 1100, 0.01, True)


def test_emd_backward_and_calc_emd(dev):
    from chamfer3D.model_utils import calc_emd
    x1, x2 = _clouds(2, 200, 3)
    a = x1.to(dev).requires_grad_(True)
    emd_mean, dist = calc_emd(a, x2.to(dev), eps=0.01, iterations=30)
    w = torch.rand(2, 200, generator=torch.Generator().manual_seed(0))
    (dist * w.to(dev)).sum().backward()
    rd, ra = emd_ref.emd_fwd(x1.numpy(), x2.numpy(), 0.01, 30)
    exp = 2 * w.numpy()[..., None] * (x1.numpy() - np.take_along_axis(x2.numpy(), ra[..., None].astype(np.int64), 1))
    np.testing.assert_allclose(a.grad.cpu().numpy(), exp, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(emd_mean.detach().cpu().numpy(), np.sqrt(rd).mean(1), rtol=1e-6)


def test_emd_backward_six_blocks(dev):
    """ured_emd_bwd at n = 1300: six blocks of 256 points, the last one partial, two batch items;
    the float64 gather 2 * w * (x1 - x2[assignment]) on the oracle's assignment."""
    from emd import emd
    b, n = 2, 1300
    x1, x2 = _clouds(b, n, 5)
    a = x1.to(dev).requires_grad_(True)
    dist, asg = emd()(a, x2.to(dev), 0.01, 30)
    w = torch.rand(b, n, generator=torch.Generator().manual_seed(0))
    (dist * w.to(dev)).sum().backward()
    rd, ra = emd_ref.emd_fwd(x1.numpy(), x2.numpy(), 0.01, 30)
    np.testing.assert_array_equal(asg.cpu().numpy(), ra)
    assert (ra >= 0).all()
    x1d, x2d, wd = (t.numpy().astype(np.float64) for t in (x1, x2, w))
    exp = 2 * wd[..., None] * (x1d - np.take_along_axis(x2d, ra[..., None].astype(np.int64), 1))
    np.testing.assert_allclose(a.grad.cpu().numpy(), exp, rtol=1e-6, atol=1e-7)


def test_emd_workspace_size_and_refusal(dev):
    """ured_emd_workspace is 24 bytes per point (0 for an empty problem); ured_emd_fwd refuses a
    workspace one byte short before any launch: dist and assignment keep their contents."""
    from ured_hip import _lib
    for b, n in [(2, 1025), (1, 1027), (2, 2048), (1, 2049), (1, 4100), (3, 5), (2, 3), (2, 70), (2, 1300), (1, 1100)]:
        assert _lib.query("ured_emd_workspace", b, n) == 24 * b * n
    for b, n in [(0, 5), (5, 0), (0, 0)]:
        assert _lib.query("ured_emd_workspace", b, n) == 0
    b, n = 2, 70
    x1, x2 = (t.to(dev) for t in _clouds(b, n, 2))
    dist = torch.full((b, n), -7.5, device=dev)
    asg = torch.full((b, n), -77, device=dev, dtype=torch.int32)
    nbytes = 24 * b * n
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.UredError, match="workspace"):
        _lib.call("ured_emd_fwd", _lib.ptr(x1), _lib.ptr(x2), b, n, 0.05, 3, _lib.ptr(dist), _lib.ptr(asg),
                  _lib.ptr(ws), nbytes - 1, _lib.stream_of(x1))
    torch.cuda.synchronize()
    assert bool((dist == -7.5).all()) and bool((asg == -77).all())
    _lib.call("ured_emd_fwd", _lib.ptr(x1), _lib.ptr(x2), b, n, 0.05, 3, _lib.ptr(dist), _lib.ptr(asg),
              _lib.ptr(ws), nbytes, _lib.stream_of(x1))
    rd, ra = emd_ref.emd_fwd(x1.cpu().numpy(), x2.cpu().numpy(), 0.05, 3)
    np.testing.assert_array_equal(asg.cpu().numpy(), ra)
    np.testing.assert_array_equal(dist.cpu().numpy(), rd)
