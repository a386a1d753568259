"""ured_hip.nn.knn (ured_knn_fwd / ured_knn_bwd), loss.basic_loss.knn_points with K > 1 and
dataset.gen_occ_point.neighbour_table against the numpy reference tests/knn_ref.py: forward
results bit-exact (the kernels and the C oracle evaluate the same fp32 formula, the order is
(distance, index)), gradients within the fp32 summation bound of the float64 reference."""
import functools

import numpy as np
import pytest
import torch

import knn_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unn(dev):
    from ured_hip import nn
    return nn


def _rand(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).random(shape, dtype=np.float32)


def _t(x, dev):
    return None if x is None else torch.from_numpy(np.array(x)).to(dev)     # a copy: the shared cases stay read-only


STREAM = [(4, 100, 200, 8), (3, 257, 129, 4), (2, 1, 5, 3), (1, 70, 1300, 16), (2, 33, 4100, 32),
          (1, 300, 300, 5), (1, 300, 300, 20), (2, 50, 7, 16),
          # the cases above split the ref range four ways (few queries); from 1024 waves of
          # queries (64 per wave) on two ways, from 2048 on not at all
          (33, 2000, 600, 12), (64, 2048, 40, 3)]
SELECT = [(1, 40, 1000, 33), (2, 257, 129, 129), (1, 300, 300, 150), (1, 64, 4096, 1024), (2, 20, 100, 300)]
# ragged (B = 4): lengths 0, n / m, below K, and a random one, on both paths
RAGGED = [(4, 100, 200, 8), (4, 60, 300, 150)]


def _points(B, n, m):
    return _rand((B, n, 3), n), _rand((B, m, 3), m + 7)


def _ragged_lengths(n, m, K):
    rng = np.random.Generator(np.random.PCG64(n + m + K))
    l1 = np.array([n, 0, n // 3, int(rng.integers(1, n))], np.int64)
    l2 = np.array([K - 3, m, int(rng.integers(K, m)), 0], np.int64)
    return l1, l2


@functools.lru_cache(maxsize=None)
def _case(B, n, m, K, ragged=False):
    """Inputs and the reference result of one case, computed once and shared (read-only)."""
    p1, p2 = _points(B, n, m)
    l1, l2 = _ragged_lengths(n, m, K) if ragged else (None, None)
    d, i = knn_ref.knn(p1, p2, K, l1, l2)
    for a in (p1, p2, d, i):
        a.setflags(write=False)
    return p1, p2, l1, l2, d, i


@pytest.mark.parametrize("B,n,m,K", STREAM + SELECT)
def test_fwd_bitexact(unn, dev, B, n, m, K):
    p1, p2, _, _, rd, ri = _case(B, n, m, K)
    d, i = unn.knn(_t(p1, dev), _t(p2, dev), K)
    assert d.shape == (B, n, K) and d.dtype == torch.float32 and i.dtype == torch.int32
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(d.cpu().numpy(), rd)


@pytest.mark.parametrize("B,n,m,K", RAGGED)
@pytest.mark.parametrize("ltype", [torch.int64, torch.int32])
def test_fwd_ragged_writes_padding(unn, dev, B, n, m, K, ltype):
    """Through the C entry point, with the output buffers pre-filled (NaN / -1): every slot is
    written, padding as (0, 0). Lengths outside [0, n] / [0, m] are clamped on the device."""
    from ured_hip import _lib
    p1, p2, l1, l2, rd, ri = _case(B, n, m, K, True)
    a, c = _t(p1, dev), _t(p2, dev)
    d = torch.full((B, n, K), float("nan"), device=dev)
    i = torch.full((B, n, K), -1, device=dev, dtype=torch.int32)
    t1, t2 = _t(l1, dev).int(), _t(l2, dev).int()
    _lib.call("ured_knn_fwd", _lib.ptr(a), _lib.ptr(c), B, n, m, K, _lib.ptr(t1), _lib.ptr(t2),
              _lib.ptr(d), _lib.ptr(i), _lib.stream_of(a))
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(d.cpu().numpy(), rd)
    # the autograd op, integer lengths of either width; n + 5 / -2 clamp to n / 0
    w1, w2 = _t(l1, dev).to(ltype), _t(l2, dev).to(ltype)
    w1 = torch.where(w1 == n, w1 + 5, w1)
    w2 = torch.where(w2 == 0, w2 - 2, w2)
    d2, i2 = unn.knn(a, c, K, w1, w2)
    np.testing.assert_array_equal(i2.cpu().numpy(), ri)
    np.testing.assert_array_equal(d2.cpu().numpy(), rd)


@pytest.mark.parametrize("K", [7, 40])
def test_ties_lowest_index(unn, dev, K):
    ax = np.linspace(0, 1, 6, dtype=np.float32)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, -1, 3)
    refs = np.concatenate([grid, grid, grid], 1)         # every distance is tied 3x
    q = np.concatenate([np.full((1, 300, 3), 0.1, np.float32), _rand((1, 200, 3), 3)], 1)
    rd, ri = knn_ref.knn(q, refs, K)
    d, i = unn.knn(_t(q, dev), _t(refs, dev), K)
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(d.cpu().numpy(), rd)


@pytest.mark.parametrize("B,n,m", [(3, 257, 129), (1, 70, 1300), (2, 300, 4100)])
def test_k1_equals_nn_dense(unn, dev, B, n, m):
    p1, p2 = _points(B, n, m)
    a, c = _t(p1, dev), _t(p2, dev)
    d, i = unn.knn(a, c, 1)
    d1, _, i1, _ = unn.nn_dense(a, c)
    assert torch.equal(d[:, :, 0], d1) and torch.equal(i[:, :, 0], i1)


def _grads(unn, dev, p1, p2, K, l1, l2, g):
    a, c = _t(p1, dev).requires_grad_(True), _t(p2, dev).requires_grad_(True)
    d, i = unn.knn(a, c, K, _t(l1, dev), _t(l2, dev))
    assert not i.requires_grad
    (d * _t(g, dev)).sum().backward()
    return a.grad, c.grad, i.cpu().numpy()


def _check_bwd(unn, dev, p1, p2, K, l1, l2, seed):
    B, n, _ = p1.shape
    g = _rand((B, n, K), seed) - 0.5
    ga, gc, idx = _grads(unn, dev, p1, p2, K, l1, l2, g)
    r1, r2, T1, S1, T2, S2 = knn_ref.knn_bwd(p1, p2, g, idx, l1, l2)     # on the kernel's own indices
    for got, ref, T, S, name in ((ga, r1, T1, S1, "grad_p1"), (gc, r2, T2, S2, "grad_p2")):
        got = got.cpu().numpy().astype(np.float64)
        tol = 2.0 * (T + 3.0) * 2.0 ** -24 * S       # fp32 summation bound of T terms, any order, x2
        err = np.abs(got - ref)
        print(name, "max err / tol", float((err / np.maximum(tol, 1e-300)).max()), "max terms", int(T.max()))
        assert (err <= tol).all(), name
        assert (got[T == 0] == 0).all(), name + ": padded rows / unreferenced points are exactly 0"
    # deterministic: a second run is bitwise identical
    ga2, gc2, _ = _grads(unn, dev, p1, p2, K, l1, l2, g)
    assert torch.equal(ga2, ga) and torch.equal(gc2, gc)
    return T2


@pytest.mark.parametrize("B,n,m,K,ragged", [(4, 100, 200, 8, False), (1, 300, 300, 150, False),
                                            (4, 100, 200, 8, True), (4, 60, 300, 150, True)])
def test_bwd(unn, dev, B, n, m, K, ragged):
    p1, p2, l1, l2, _, _ = _case(B, n, m, K, ragged)
    _check_bwd(unn, dev, p1, p2, K, l1, l2, 17)
    if ragged:      # rows beyond lengths1 / points beyond lengths2: exactly 0 (also asserted through T == 0)
        ga, gc, _ = _grads(unn, dev, p1, p2, K, l1, l2, np.ones((B, n, K), np.float32))
        for b in range(B):
            assert float(ga[b, int(l1[b]):].abs().sum()) == 0.0 and float(gc[b, int(l2[b]):].abs().sum()) == 0.0


def test_bwd_degenerate_in_degree(unn, dev):
    """One ref is every query's nearest (in-degree n = 3000: a contribution list of several LDS
    tiles for one point)."""
    n, K = 3000, 4
    p1 = _rand((1, n, 3), 21)
    p2 = np.concatenate([np.full((1, 1, 3), 0.5, np.float32), 10.0 + _rand((1, 8, 3), 22)], 1)
    T2 = _check_bwd(unn, dev, p1, p2, K, None, None, 23)
    assert int(T2[0, 0, 0]) == n


def test_knn_points(dev):
    from loss.basic_loss import knn_points
    from ured_hip.nn import nn_segments
    B, n, m, K = 3, 50, 80, 5
    p1, p2 = _points(B, n, m)
    a, c = _t(p1, dev), _t(p2, dev).requires_grad_(True)
    l2 = np.array([80, 3, 40], np.int64)
    rd, ri = knn_ref.knn(p1, p2, K, None, l2)
    r = knn_points(a, c, lengths2=_t(l2, dev), K=K, return_nn=True, return_sorted=False)
    assert r.idx.dtype == torch.int64 and r.idx.shape == (B, n, K) and r.knn.shape == (B, n, K, 3)
    np.testing.assert_array_equal(r.idx.cpu().numpy(), ri)              # lengths2 honoured
    np.testing.assert_array_equal(r.dists.detach().cpu().numpy(), rd)
    want = p2[np.arange(B)[:, None, None], ri] * (np.arange(K) < l2[:, None, None])[..., None]
    np.testing.assert_array_equal(r.knn.detach().cpu().numpy(), want)   # p2 gathered through idx
    w = _t(_rand((B, n, K, 3), 9) - 0.5, dev)
    (r.knn * w).sum().backward()                                        # gradient flows through knn
    gref = np.zeros_like(p2)
    valid = np.broadcast_to((np.arange(K) < l2[:, None, None]), ri.shape)
    for b in range(B):
        np.add.at(gref[b], ri[b][valid[b]], w[b].cpu().numpy()[valid[b]])
    np.testing.assert_allclose(c.grad.cpu().numpy(), gref, rtol=1e-5, atol=1e-6)
    assert knn_points(a, c, K=K).knn is None
    # K = 1: bitwise the ragged nearest-neighbour launch it has always been
    valid2 = _t(l2, dev)
    k1 = knn_points(a, c.detach(), lengths2=valid2, K=1, return_nn=True)
    ar = torch.arange(B, device=dev)
    segs = torch.stack([ar * m, valid2, ar * n, torch.full_like(ar, n)], 1).int()
    _, _, d, i = nn_segments(c.detach().contiguous(), a.contiguous(), segs, m, n, 2)
    assert torch.equal(k1.dists, d.view(B, n, 1)) and torch.equal(k1.idx, i.view(B, n, 1).long())
    assert torch.equal(k1.knn, torch.gather(c.detach(), 1, k1.idx.expand(-1, -1, 3)).unsqueeze(2))
    with pytest.raises(NotImplementedError):
        knn_points(a, c, K=K, norm=1)
    with pytest.raises(NotImplementedError):
        knn_points(a, c, K=1, norm=1)


@pytest.mark.parametrize("N", [64, 300])
def test_neighbour_table(dev, N):
    from dataset.gen_occ_point import neighbour_table
    x = _rand((2, N, 3), N)
    _, ri = knn_ref.knn(x, x, N // 2)
    tab = neighbour_table(_t(x, dev))
    assert tab.dtype == torch.int64 and tab.shape == (2, N, N // 2)
    np.testing.assert_array_equal(tab.cpu().numpy(), ri)
    np.testing.assert_array_equal(tab[:, :, 0].cpu().numpy(), np.broadcast_to(np.arange(N), (2, N)))
    one = neighbour_table(_t(x[1], dev))
    assert one.shape == (N, N // 2) and torch.equal(one, tab[1])


def test_graph_capture(unn, dev):
    """The forward is capturable (no allocation in the library, no host sync, the caller's
    stream): a replay on new inputs equals the eager result. Single stream, no branches."""
    B, n, m, K = 2, 100, 200, 8
    p1, p2 = _points(B, n, m)
    a, c = _t(p1, dev), _t(p2, dev)
    unn.knn(a, c, K)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d, i = unn.knn(a, c, K)
    a.copy_(_t(_rand((B, n, 3), 71), dev))
    c.copy_(_t(_rand((B, m, 3), 72), dev))
    g.replay()
    torch.cuda.synchronize()
    de, ie = unn.knn(a, c, K)
    assert torch.equal(d, de) and torch.equal(i, ie)
    rd, ri = knn_ref.knn(a.cpu().numpy(), c.cpu().numpy(), K)
    np.testing.assert_array_equal(i.cpu().numpy(), ri)


def test_errors_raise(unn, dev):
    from ured_hip import _lib
    a, c = torch.rand(2, 5, 3, device=dev), torch.rand(2, 7, 3, device=dev)
    with pytest.raises(RuntimeError):
        unn.knn(torch.rand(2, 5, 3), torch.rand(2, 5, 3), 2)          # CPU tensors: no fallback
    with pytest.raises(_lib.UredError, match="1024"):
        unn.knn(a, c, 0)
    with pytest.raises(_lib.UredError, match="1024"):
        unn.knn(a, c, 1025)
    with pytest.raises(_lib.UredError, match="4096"):
        unn.knn(a, torch.rand(2, 4097, 3, device=dev), 33)
    with pytest.raises(TypeError):
        unn.knn(a.double(), c, 2)
    with pytest.raises(ValueError):
        unn.knn(a, c[:, :, :2], 2)
    with pytest.raises(ValueError):
        unn.knn(a, c[:1], 2)
    with pytest.raises(ValueError):
        unn.knn(a[0], c[0], 2)
    with pytest.raises(ValueError):
        unn.knn(a, c, 2, lengths2=torch.tensor([1.0, 2.0], device=dev))
    with pytest.raises(ValueError):
        unn.knn(a, c, 2, lengths1=torch.tensor([1, 2, 3], device=dev))
    with pytest.raises(RuntimeError):
        unn.knn(a, c, 2, lengths2=torch.tensor([1, 2]))
