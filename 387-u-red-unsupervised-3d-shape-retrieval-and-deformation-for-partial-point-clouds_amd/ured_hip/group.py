"""PointNet++ set abstraction primitives on the device (csrc/group.hip): farthest-point sampling,
ball query and grouping, the torch compositions of the reference's network/pointnet/
pointnet2_utils.py:63-138 as one launch each (two for the grouping's backward). Indices are int32
here, as in knn(); network/pointnet/pointnet2_utils.py hands out the reference's int64. No CPU
fallback."""
import ctypes

import torch
from torch.autograd import Function

from . import _lib

FPS_NMAX = 16384                  # URED_FPS_NMAX (include/ured_hip.h)
MAX_B = 65535
_LIM = 1 << 31

_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_lib.register({
    "ured_fps": [_P, _P, _I, _I, _I, _P, _P],
    "ured_ball_query": [_P, _P, _I, _I, _I, _F, _I, _P, _P],
    "ured_group_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    "ured_group_bwd": [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P],
})


def _cloud(who, name, t, B=None, C=3):
    """t must be a float32 [B, *, C] device tensor -> (B, rows)."""
    if t.dim() != 3 or (C is not None and t.shape[-1] != C):
        raise ValueError(f"{who}: {name} must be [B,N,{C if C is not None else 'D'}], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")
    if B is not None and t.shape[0] != B:
        raise ValueError(f"{who}: {name} has batch {t.shape[0]}, expected {B}")
    return t.shape[0], t.shape[1]


def _same_device(who, ref, **others):
    for name, t in others.items():
        if t is not None and t.device != ref.device:
            raise ValueError(f"{who}: {name} is on {t.device}, expected {ref.device}")


def _limits(who, B, N, S, K, D):
    if B > MAX_B:
        raise ValueError(f"{who}: B {B} exceeds {MAX_B}")
    if N < 1:
        raise ValueError(f"{who}: N {N} must be at least 1")
    if K < 1:
        raise ValueError(f"{who}: the group size {K} must be at least 1")
    if B * N * max(D, 3) >= _LIM or B * S * K * (3 + D) >= _LIM:
        raise ValueError(f"{who}: B * N * max(D, 3) and B * S * K * (3 + D) must stay below 2^31 "
                         f"(B={B} N={N} S={S} K={K} D={D})")


def fps(xyz, npoint, start=None):
    """Farthest-point sampling. xyz [B,N,3] fp32, 1 <= N <= 16384 -> int32 [B,npoint]: column 0 is
    `start` (int tensor [B] on the device, clamped into [0,N) by the kernel; None draws
    torch.randint(0, N, (B,)) on the device), column i + 1 the lowest index among the points farthest
    from columns 0..i, by d = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32. npoint > N is allowed."""
    _lib.require_device(xyz, start)
    B, N = _cloud("fps", "xyz", xyz)
    npoint = int(npoint)
    if not 1 <= N <= FPS_NMAX:
        raise ValueError(f"fps: N {N} outside [1, {FPS_NMAX}]")
    if npoint < 1:
        raise ValueError(f"fps: npoint {npoint} must be at least 1")
    if B > MAX_B or B * npoint >= _LIM:
        raise ValueError(f"fps: B {B} exceeds {MAX_B} or B * npoint reaches 2^31")
    if start is None:
        start = torch.randint(0, N, (B,), device=xyz.device, dtype=torch.int32)
    else:
        if tuple(start.shape) != (B,) or start.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"fps: start must be int32 / int64 [{B}], got {start.dtype} {tuple(start.shape)}")
        _same_device("fps", xyz, start=start)
        start = start.to(torch.int32).contiguous()
    xyz = xyz.contiguous()
    out = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
    _lib.call("ured_fps", _lib.ptr(xyz), _lib.ptr(start), B, N, npoint, _lib.ptr(out), _lib.stream_of(xyz))
    return out


def ball_query(radius, nsample, xyz, new_xyz):
    """xyz [B,N,3], new_xyz [B,S,3] fp32 -> int32 [B,S,nsample]: per query the first nsample point
    indices, ascending, whose squared distance is not above float32(radius ** 2) (boundary included);
    shorter rows padded with their first index; rows without a hit hold N."""
    _lib.require_device(xyz, new_xyz)
    B, N = _cloud("ball_query", "xyz", xyz)
    _, S = _cloud("ball_query", "new_xyz", new_xyz, B)
    _same_device("ball_query", xyz, new_xyz=new_xyz)
    nsample = int(nsample)
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError(f"ball_query: radius {radius} must be non-negative")
    _limits("ball_query", B, N, S, nsample, 0)
    xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
    out = torch.empty(B, S, nsample, dtype=torch.int32, device=xyz.device)
    r2 = float(torch.tensor(radius * radius, dtype=torch.float32))   # radius ** 2 rounded to fp32, as the reference's mask
    _lib.call("ured_ball_query", _lib.ptr(xyz), _lib.ptr(new_xyz), B, N, S, r2, nsample, _lib.ptr(out),
              _lib.stream_of(xyz))
    return out


class GroupFn(Function):
    """(xyz [B,N,3] | None, new_xyz [B,S,3] | None, points [B,N,D] | None, idx int32 [B,S,K]) ->
    out [B*S*K, 3 + D] point-major (what the conv chain reads): columns 0..2 = xyz[idx] - new_xyz[s],
    the rest points[idx]; without xyz / new_xyz a plain gather [B*S*K, D]. An index outside [0,N)
    gives a zero row and no gradient. idx is not differentiable. The backward writes every gradient
    with sums in ascending (s,k) order: deterministic, no atomics."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, points, idx):
        who = "GroupFn"
        _lib.require_device(xyz, new_xyz, points, idx)
        if (xyz is None) != (new_xyz is None):
            raise ValueError(f"{who}: xyz and new_xyz go together")
        if xyz is None and points is None:
            raise ValueError(f"{who}: nothing to gather")
        if idx.dim() != 3 or idx.dtype != torch.int32:
            raise ValueError(f"{who}: idx must be int32 [B,S,K], got {idx.dtype} {tuple(idx.shape)}")
        B, S, K = idx.shape
        D = 0
        if xyz is not None:
            _, N = _cloud(who, "xyz", xyz, B)
            _, S2 = _cloud(who, "new_xyz", new_xyz, B)
            if S2 != S:
                raise ValueError(f"{who}: new_xyz has {S2} rows, idx {S}")
        if points is not None:
            _, Np = _cloud(who, "points", points, B, C=None)
            D = points.shape[2]
            if D < 1:
                raise ValueError(f"{who}: points has no channels")
            if xyz is not None and Np != N:
                raise ValueError(f"{who}: points has {Np} rows, xyz {N}")
            N = Np
        ref = xyz if xyz is not None else points
        _same_device(who, ref, new_xyz=new_xyz, points=points, idx=idx)
        _limits(who, B, N, S, K, D)
        c3 = 3 if xyz is not None else 0
        xyz_c = None if xyz is None else xyz.contiguous()
        new_c = None if new_xyz is None else new_xyz.contiguous()
        pts_c = None if points is None else points.contiguous()
        idx = idx.contiguous()
        out = torch.empty(B * S * K, c3 + D, device=ref.device)
        _lib.call("ured_group_fwd", _lib.ptr(xyz_c), _lib.ptr(new_c), _lib.ptr(pts_c), _lib.ptr(idx), B, N, S, K, D,
                  _lib.ptr(out), _lib.stream_of(ref))
        ctx.save_for_backward(idx)
        ctx.dims = (B, N, S, K, D, c3)
        return out

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        B, N, S, K, D, c3 = ctx.dims
        g = g.contiguous()
        dev = g.device
        gx = gn = gp = None
        if c3:   # written in full by the kernels, as is gp
            gx, gn = torch.empty(B, N, 3, device=dev), torch.empty(B, S, 3, device=dev)
        if D:
            gp = torch.empty(B, N, D, device=dev)
        _lib.call("ured_group_bwd", _lib.ptr(g), _lib.ptr(idx), B, N, S, K, D, _lib.ptr(gx), _lib.ptr(gn), _lib.ptr(gp),
                  _lib.stream_of(g))
        need = ctx.needs_input_grad
        return (gx if need[0] else None, gn if need[1] else None, gp if need[2] else None, None)

