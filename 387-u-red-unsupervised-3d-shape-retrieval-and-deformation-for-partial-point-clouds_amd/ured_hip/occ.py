"""Partial (occluded) target clouds on the device: ured_occlude (csrc/occ.hip), the reference's
dataset/gen_occ_point.py + the centring / random rotation of partnet_dataset.py:45-78 as one
launch for a whole batch. No CPU fallback."""
import ctypes

import torch

from . import _lib

PLAN_I, PLAN_F = 12, 6            # URED_OCC_PLAN_I / _F (include/ured_hip.h)
MODE_BALL, MODE_RANDOM, MODE_SLICE, MODE_PART = 0, 1, 2, 3
MIN_N, MAX_N = 16, 4096

_P, _I, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
_lib.register({"ured_occlude": [_P, _P, _P, _I, _I, _U64, _U64, _P, _I, _P, _P, _I] + [_P] * 10})


def occlude(x, labels, sem, seed, step=0, modes=None, plan=None, rotate=False):
    """x [B,N,3] fp32, labels / sem [B,N] int64 (device tensors), 16 <= N <= 4096 -> dict of
      mask int64 [B,K] (K = N // 2 kept point indices, ascending), ori_point_occ [B,K,3] = x[mask],
      point_occ [B,K,3] (centred, rotated iff `rotate`), labels_occ / sem_occ [B,K], occ_mean [B,3],
      occ_rot [B,3,3] (point_occ = (occ_rot @ (ori - mean)^T)^T; identity without rotation),
      plan_i int32 [B,12], plan_f fp32 [B,6]: the plan used (layout: include/ured_hip.h).
    Stateless: the same (seed, step) gives the same bits. `modes` (one int, or an int tensor / list [B];
    -1 = draw, 0..3) forces the occlusion mode; `plan` = (plan_i, plan_f) replaces the whole drawn plan."""
    _lib.require_device(x, labels, sem)
    if x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError(f"occlude: x must be [B,N,3], got {tuple(x.shape)}")
    B, N, _ = x.shape
    if not MIN_N <= N <= MAX_N:
        raise ValueError(f"occlude: N {N} outside [{MIN_N}, {MAX_N}]")
    if x.dtype != torch.float32:
        raise ValueError(f"occlude: x must be float32, got {x.dtype}")
    for name, v in (("labels", labels), ("sem", sem)):
        if tuple(v.shape) != (B, N) or v.dtype != torch.int64:
            raise ValueError(f"occlude: {name} must be int64 [{B},{N}], got {v.dtype} {tuple(v.shape)}")
        if v.device != x.device:
            raise ValueError(f"occlude: {name} is on {v.device}, x on {x.device}")
    if modes is not None and plan is not None:
        raise ValueError("occlude: a plan carries its mode; give modes or plan, not both")
    dev = x.device
    m = pi = pf = None
    mode_all = -1
    if modes is not None:
        if isinstance(modes, int):                    # one mode for the batch: an argument, no upload
            if not -1 <= modes <= 3:
                raise ValueError(f"occlude: mode {modes} outside [-1, 3]")
            mode_all = modes
        elif torch.is_tensor(modes) and modes.is_cuda:
            m = modes.to(torch.int32).contiguous()    # device values above 3 are clamped by the kernel
        else:
            host = torch.as_tensor(modes, dtype=torch.int32)
            if host.numel() and (int(host.min()) < -1 or int(host.max()) > 3):
                raise ValueError(f"occlude: modes outside [-1, 3]: {host.tolist()}")
            m = host.to(dev)
        if m is not None and tuple(m.shape) != (B,):
            raise ValueError(f"occlude: modes must have {B} entries, got {tuple(m.shape)}")
    if plan is not None:
        pi, pf = plan
        _lib.require_device(pi, pf)
        if tuple(pi.shape) != (B, PLAN_I) or pi.dtype != torch.int32 or tuple(pf.shape) != (B, PLAN_F) \
                or pf.dtype != torch.float32:
            raise ValueError(f"occlude: plan must be (int32 [{B},{PLAN_I}], float32 [{B},{PLAN_F}])")
        pi, pf = pi.contiguous(), pf.contiguous()
    x, labels, sem = x.contiguous(), labels.contiguous(), sem.contiguous()
    K = N // 2
    # four allocations for the ten outputs (the loaders call this once per batch)
    i64 = torch.empty(3, B, K, dtype=torch.int64, device=dev)
    pts = torch.empty(2, B, K, 3, device=dev)
    small = torch.empty(B * (3 + 9 + PLAN_F), device=dev)
    o = dict(mask=i64[0], ori_point_occ=pts[0], point_occ=pts[1], labels_occ=i64[1], sem_occ=i64[2],
             occ_mean=small[:3 * B].view(B, 3), occ_rot=small[3 * B:12 * B].view(B, 3, 3),
             plan_i=torch.empty(B, PLAN_I, dtype=torch.int32, device=dev), plan_f=small[12 * B:].view(B, PLAN_F))
    mask64 = (1 << 64) - 1
    _lib.call("ured_occlude", _lib.ptr(x), _lib.ptr(labels), _lib.ptr(sem), B, N, int(seed) & mask64,
              int(step) & mask64, _lib.ptr(m), mode_all, _lib.ptr(pi), _lib.ptr(pf), int(bool(rotate)), _lib.ptr(o["mask"]),
              _lib.ptr(o["ori_point_occ"]), _lib.ptr(o["point_occ"]), _lib.ptr(o["labels_occ"]), _lib.ptr(o["sem_occ"]),
              _lib.ptr(o["occ_mean"]), _lib.ptr(o["occ_rot"]), _lib.ptr(o["plan_i"]), _lib.ptr(o["plan_f"]),
              _lib.stream_of(x))
    return o
