"""Drop-in for the reference loss/basic_loss.py: residual_retrieval_loss (basic_loss.py:249-265)
and a stand-in for pytorch3d.ops.knn_points.

pytorch3d is absent from the reference tree (version unpinned, not importable here: the
semantics are taken from its documented contract and the boundary stays parity-unpinned); the
K=1 query here is the x -> source direction of the same HIP nearest-neighbour primitive
(squared L2, lowest index on ties), one ragged launch for the whole batch; K > 1 is
ured_hip.nn.knn (the same distance, the same tie rule).
"""
from collections import namedtuple

import torch

from ured_hip.nn import knn, nn_segments

NP_PER_PART = 1024
KNN = namedtuple("KNN", ["dists", "idx", "knn"])


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False,
               return_sorted=True, **_):
    """The K nearest neighbours of every p1 point among p2 (pytorch3d.ops.knn_points).

    p1 [B,n,3], p2 [B,m,3]; lengths1 / lengths2 [B] limit the valid points per sample.
    Returns dists [B,n,K] (squared L2), idx [B,n,K] (int64), knn [B,n,K,3] if return_nn, sorted by
    (distance, index) whatever `return_sorted` says (False permits any order); padded slots
    (beyond lengths2, rows beyond lengths1) hold 0. `version` selects among pytorch3d's kernels
    and has no meaning here. 1 <= K <= 1024; K > 32 needs m <= 4096 (ured_hip.nn.knn).
    """
    if norm != 2:
        raise NotImplementedError("only norm=2 (squared L2) is implemented")
    if K != 1:
        dev = p1.device
        l1 = None if lengths1 is None else lengths1.to(dev)
        l2 = None if lengths2 is None else lengths2.to(dev)
        d, i = knn(p1, p2, K, l1, l2)
        i = i.long()
        nn = None
        if return_nn:
            B, n, _ = p1.shape
            nn = torch.gather(p2, 1, i.reshape(B, n * K, 1).expand(-1, -1, 3)).view(B, n, K, 3)
            if l2 is not None:       # padded slots read 0, as pytorch3d's knn_gather leaves them
                nn = nn * (torch.arange(K, device=dev) < l2.view(B, 1, 1)).unsqueeze(-1)
        return KNN(d, i, nn)
    B, n, _ = p1.shape
    m = p2.shape[1]
    dev = p1.device
    ar = torch.arange(B, device=dev)
    n1 = torch.full_like(ar, n) if lengths1 is None else lengths1.to(dev).long()
    n2 = torch.full_like(ar, m) if lengths2 is None else lengths2.to(dev).long()
    segs = torch.stack([ar * m, n2, ar * n, n1], 1).int()
    _, _, d, i = nn_segments(p2.contiguous(), p1.contiguous(), segs, m, n, 2)
    d, i = d.view(B, n, 1), i.view(B, n, 1).long()
    nn = torch.gather(p2, 1, i.expand(-1, -1, 3)).unsqueeze(2) if return_nn else None
    return KNN(d, i, nn)


def residual_retrieval_loss(x, x_source, residuals, mask_part=None, np_per_part=NP_PER_PART, nn_idx=None):
    """x [B,N,3] target, x_source [B,S,3] deformed sources (only the first k_b*1024 are valid),
    residuals [B,N,3] -> (mean_n sum_xyz |x + r - nn|, mean_n sum_xyz |r|).
    nn_idx [B,N] (optional): the x -> x_source nearest-neighbour indices when the caller already
    has them (the chamfer full family computes exactly this query, compute_cm_loss(return_idx))."""
    B, S, _ = x_source.shape
    if nn_idx is None:
        valid = (mask_part.sum(1).round().long() * np_per_part).clamp(max=S)
        _, _, nn = knn_points(x, x_source, lengths2=valid, K=1, return_nn=True)
        nn = nn.squeeze(2)
    else:
        nn = torch.gather(x_source, 1, nn_idx.long().unsqueeze(-1).expand(-1, -1, 3))
    res_nn = x + residuals - nn
    return torch.abs(res_nn).sum(-1).mean(), torch.abs(residuals).sum(-1).mean()
