"""numpy reference of ured_hip.nn.knn — TEST INFRASTRUCTURE ONLY.

Distances are the exact fp32 contract distances of the C oracle (oracle/nn_oracle.c through
oracle.nn_ref.nn_dir, one ref at a time), the order is a stable argsort of them (ascending
(distance, index)), padding as documented in include/ured_hip.h (ured_knn_fwd).
"""
import numpy as np

from oracle import nn_ref


def dmat(q, r):
    """q [nq,3], r [nr,3] -> D [nq,nr] fp32, D[i,j] = fmaf(dz,dz, fmaf(dy,dy, dx*dx)), dx = r_j - q_i."""
    q, r = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(r, np.float32)
    D = np.empty((q.shape[0], r.shape[0]), np.float32)
    for j in range(r.shape[0]):
        D[:, j] = nn_ref.nn_dir(q, r[j:j + 1])[0]
    return D


def _lens(lens, B, cap):
    if lens is None:
        return np.full(B, cap, np.int64)
    return np.clip(np.asarray(lens, np.int64), 0, cap)


def knn(p1, p2, K, len1=None, len2=None):
    """p1 [B,n,3], p2 [B,m,3] -> dists [B,n,K] fp32, idx [B,n,K] int32."""
    B, n, _ = p1.shape
    m = p2.shape[1]
    l1, l2 = _lens(len1, B, n), _lens(len2, B, m)
    dists = np.zeros((B, n, K), np.float32)
    idx = np.zeros((B, n, K), np.int32)
    for b in range(B):
        a, c = int(l1[b]), int(l2[b])
        if a == 0 or c == 0:
            continue
        D = dmat(p1[b, :a], p2[b, :c])
        k = min(K, c)
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        idx[b, :a, :k] = order
        dists[b, :a, :k] = np.take_along_axis(D, order, 1)
    return dists, idx


def knn_bwd(p1, p2, gd, idx, len1=None, len2=None):
    """float64 gradients of sum(gd * dists) from a GIVEN idx [B,n,K] (valid slots only).
    -> (g1 [B,n,3], g2 [B,m,3], T1, S1, T2, S2): per output element the number of summed terms
    T and the sum of their absolute values S (for a summation error bound)."""
    B, n, _ = p1.shape
    m = p2.shape[1]
    K = idx.shape[2]
    l1, l2 = _lens(len1, B, n), _lens(len2, B, m)
    P1, P2, G = p1.astype(np.float64), p2.astype(np.float64), gd.astype(np.float64)
    g1, g2 = np.zeros((B, n, 3)), np.zeros((B, m, 3))
    T1, S1 = np.zeros((B, n, 3)), np.zeros((B, n, 3))
    T2, S2 = np.zeros((B, m, 3)), np.zeros((B, m, 3))
    for b in range(B):
        V = (np.arange(n)[:, None] < l1[b]) & (np.arange(K)[None, :] < min(K, int(l2[b])))
        if not V.any():
            continue
        ii, kk = np.nonzero(V)
        jj = idx[b, ii, kk].astype(np.int64)
        assert (jj >= 0).all() and (jj < l2[b]).all()
        term = 2.0 * G[b, ii, kk][:, None] * (P1[b, ii] - P2[b, jj])     # [E,3]
        np.add.at(g1[b], ii, term)
        np.add.at(S1[b], ii, np.abs(term))
        np.add.at(T1[b], ii, 1.0)
        np.add.at(g2[b], jj, -term)
        np.add.at(S2[b], jj, np.abs(term))
        np.add.at(T2[b], jj, 1.0)
    return g1, g2, T1, S1, T2, S2
