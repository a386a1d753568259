"""The reference's dataset/gen_occ_point.py names on the device: each is a forced-mode call of
ured_hip.occ.occlude (one HIP launch for the whole batch) and returns (occ_points, mask) like the
reference. Differences: `points` is a device tensor [N,3] or [B,N,3] (16 <= N <= 4096;
the reference asserts 2048), the mask is in ascending index order for every mode, ball occlusion
runs on every call (no on-disk kNN cache; `ids` / `save_pth` are accepted and unused), and the
draws come from `seed` (a counter-based hash, not numpy's global state)."""
import torch

from ured_hip import occ as _occ


def _forced(points, mode, seed, step, semantics=None):
    single = points.dim() == 2
    x = points.unsqueeze(0) if single else points
    if semantics is None:
        sem = torch.zeros(x.shape[:2], dtype=torch.int64, device=x.device)
    else:
        sem = (semantics.unsqueeze(0) if single else semantics).long()
    r = _occ.occlude(x, sem, sem, seed, step, modes=mode)
    pts, mask = r["ori_point_occ"], r["mask"]
    return (pts[0], mask[0]) if single else (pts, mask)


def generate_occ_point_ball(points, ids=None, save_pth="", seed=0, step=0):
    return _forced(points, _occ.MODE_BALL, seed, step)


def generate_occ_point_slice(points, seed=0, step=0):
    return _forced(points, _occ.MODE_SLICE, seed, step)


def generate_occ_point_random(points, seed=0, step=0):
    return _forced(points, _occ.MODE_RANDOM, seed, step)


def generate_occ_point_part(points, semantics, seed=0, step=0):
    return _forced(points, _occ.MODE_PART, seed, step, semantics)


def neighbour_table(points):
    """The `dis_mat` table the reference's ball occlusion builds and caches per target
    (gen_occ_point.py:31-33: knn_points(points, points, K=N // 2, return_sorted=True).idx): for
    every point the indices of its N // 2 nearest points of the same cloud (itself first, unless
    a duplicate with a lower index precedes it), ascending in (distance, index). points [N,3] or
    [B,N,3] on the device, N <= 4096 -> int64 [..., N, N // 2]. The occlusion kernel does not need
    the table; it is for sharing caches with the reference pipeline."""
    from ured_hip import nn as _nn
    single = points.dim() == 2
    x = points.unsqueeze(0) if single else points
    N = x.shape[1]
    if N < 2 or N > _nn.KNN_SEL_M:
        raise ValueError(f"neighbour_table: N {N} outside [2, {_nn.KNN_SEL_M}]")
    idx = _nn.knn(x.detach(), x.detach(), N // 2)[1].long()
    return idx[0] if single else idx
