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
