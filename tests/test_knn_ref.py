"""The numpy kNN reference (tests/knn_ref.py) against a float64 brute force, its tie and padding
rules, and the argument checks of ured_knn_fwd / ured_knn_bwd (no GPU needed: validation happens
before any device work)."""
import numpy as np
import pytest

import knn_ref
from oracle import nn_ref


def _rand(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).random(shape, dtype=np.float32)


def _lattice3():
    ax = np.linspace(0, 1, 6, dtype=np.float32)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([grid, grid, grid], 0)


@pytest.mark.parametrize("n,m,K", [(100, 200, 8), (257, 129, 129), (300, 300, 150), (64, 4100, 16)])
def test_ref_equals_float64_brute_force(n, m, K):
    """Indices: exactly a float64 brute-force stable argsort (these inputs have no fp32 tie inside
    any top K+1, so the fp32 order is the float64 order). Distances: within 5 * 2^-24 relative of
    float64 (three input roundings doubled by squaring, plus two fused roundings)."""
    p1, p2 = _rand((n, 3), n), _rand((m, 3), m + 7)
    d, i = knn_ref.knn(p1[None], p2[None], K)
    q, r = p1.astype(np.float64), p2.astype(np.float64)
    D64 = ((r[None] - q[:, None]) ** 2).sum(-1)
    order = np.argsort(D64, axis=1, kind="stable")
    top = np.take_along_axis(knn_ref.dmat(p1, p2), order[:, :min(K + 1, m)], 1)
    assert (np.diff(top, axis=1) != 0).all(), "fp32 tie inside a top K+1"
    assert int((i[0] != order[:, :K]).any(1).sum()) == 0
    d64 = np.take_along_axis(D64, order[:, :K], 1)
    rel = np.abs(d[0].astype(np.float64) - d64) / d64
    print("max relative distance error", rel.max())
    assert rel.max() <= 5 * 2.0 ** -24


def test_column0_is_nn_dir():
    p1, p2 = _rand((257, 3), 257), _rand((129, 3), 136)
    d, i = knn_ref.knn(p1[None], p2[None], 5)
    rd, ri = nn_ref.nn_dir(p1, p2)
    np.testing.assert_array_equal(d[0, :, 0], rd)
    np.testing.assert_array_equal(i[0, :, 0], ri)


def test_ties_indices_ascend():
    refs = _lattice3()
    q = np.concatenate([np.full((300, 3), 0.1, np.float32), _rand((200, 3), 3)], 0)
    d, i = knn_ref.knn(q[None], refs[None], 7)
    d, i = d[0], i[0]
    assert (np.diff(d, axis=1) >= 0).all()
    tied = np.diff(d, axis=1) == 0
    assert tied.sum() >= 2 * len(q)                        # every distance comes three times
    assert (np.diff(i, axis=1)[tied] > 0).all()            # among equal distances the indices ascend
    # the random queries: the three copies of the nearest lattice point, lowest copy first
    np.testing.assert_array_equal(i[300:, 1], i[300:, 0] + 216)
    np.testing.assert_array_equal(i[300:, 2], i[300:, 0] + 432)


def test_padding_rule():
    p1, p2 = _rand((3, 20, 3), 1), _rand((3, 7, 3), 2)
    d, i = knn_ref.knn(p1, p2, 16)                         # K > m
    assert (d[:, :, 7:] == 0).all() and (i[:, :, 7:] == 0).all()
    assert (np.sort(i[:, :, :7], axis=2) == np.arange(7)).all()
    l1, l2 = np.array([20, 0, 5]), np.array([3, 7, 0])
    d, i = knn_ref.knn(p1, p2, 4, l1, l2)
    assert (d[0, :, 3:] == 0).all() and (i[0, :, 3:] == 0).all() and (i[0, :, :3] < 3).all()
    assert (d[0, :, :3] > 0).all()
    assert (d[1] == 0).all() and (i[1] == 0).all()         # no valid query
    assert (d[2] == 0).all() and (i[2] == 0).all()         # no valid ref
    d5, i5 = knn_ref.knn(p1[2:, :5], p2[2:], 4)
    d, i = knn_ref.knn(p1, p2, 4, np.array([20, 20, 5]), None)
    np.testing.assert_array_equal(d[2, :5], d5[0])
    assert (d[2, 5:] == 0).all() and (i[2, 5:] == 0).all()


def test_bwd_ref_counts_terms():
    p1, p2 = _rand((1, 6, 3), 5), _rand((1, 4, 3), 6)
    _, i = knn_ref.knn(p1, p2, 2)
    g = _rand((1, 6, 2), 7) - 0.5
    g1, g2, T1, S1, T2, S2 = knn_ref.knn_bwd(p1, p2, g, i)
    assert (T1 == 2).all() and T2.sum() == 3 * 12
    np.testing.assert_allclose(g1.sum(1), -g2.sum(1), rtol=1e-12, atol=1e-15)
    assert (np.abs(g1) <= S1).all() and (np.abs(g2) <= S2).all()


def test_knn_abi_limits_without_gpu(built):
    from ured_hip import _lib
    fwd = lambda b, n, m, K: _lib.call("ured_knn_fwd", None, None, b, n, m, K, None, None, None, None, None)
    bwd = lambda b, n, m, K: _lib.call("ured_knn_bwd", None, None, b, n, m, K, None, None, None, None, None, None, None)
    for call in (fwd, bwd):
        with pytest.raises(_lib.UredError, match=r"K 0 outside \[1, 1024\]"):
            call(1, 4, 4, 0)
        with pytest.raises(_lib.UredError, match=r"K 1025 outside \[1, 1024\]"):
            call(1, 4, 4, 1025)
        with pytest.raises(_lib.UredError, match=r"K 33 > 32 needs m <= 4096"):
            call(1, 4, 4097, 33)
        with pytest.raises(_lib.UredError, match="negative size"):
            call(1, -1, 4, 2)
        # NULL pointers at valid sizes raise rather than crash
        for K, m in ((1, 4), (8, 5000), (33, 4096), (1024, 100)):
            with pytest.raises(_lib.UredError, match="null pointer"):
                call(2, 4, m, K)
        call(0, 4, 4, 1)         # an empty batch is no error (and clears the thread's message)
    assert _lib.lib().ured_last_error() == b""
