"""PointNet++ feature propagation on the device (csrc/interp.hip): the three nearest coarse points
of every fine point (ured_hip.nn.knn) and the inverse-distance interpolation of the coarse features
over them, written with the skip features as the point-major matrix the conv chain reads: the
sort / advanced indexing / weighted sum / cat of the reference's network/pointnet/
pointnet2_utils.py:293-309 as one launch (two for the backward). No CPU fallback."""
import ctypes

import torch
from torch.autograd import Function

from . import _lib
from .group import MAX_B, _LIM, _cloud, _same_device
from .nn import knn

MAX_K = 3

_P, _I = ctypes.c_void_p, ctypes.c_int
_lib.register({
    "ured_interp_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_interp_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P],
})


def three_nn(xyz1, xyz2):
    """xyz1 [B,N,3] fine, xyz2 [B,S,3] coarse -> (d2 [B,N,K] squared distances, idx int32 [B,N,K]),
    K = min(3, S): knn(xyz1, xyz2, K), ascending in (distance, index), differentiable in both clouds.
    Never more columns than S: knn pads with (0, 0), which would read as a coincident neighbour."""
    _lib.require_device(xyz1, xyz2)
    B, _ = _cloud("three_nn", "xyz1", xyz1)
    _, S = _cloud("three_nn", "xyz2", xyz2, B)
    _same_device("three_nn", xyz1, xyz2=xyz2)
    if S < 1:
        raise ValueError("three_nn: xyz2 has no points")
    return knn(xyz1, xyz2, min(MAX_K, S))


class InterpFn(Function):
    """(points1 [B,N,D1] | None, points2 [B,S,D2], idx int32 [B,N,K], d2 [B,N,K]), 1 <= K <= 3 ->
    out [B*N, D1 + D2] point-major: columns 0..D1-1 = points1, the rest the interpolation
    sum_k w_k points2[b, idx[b,n,k]], w_k = r_k / sum_j r_j, r_k = 1 / (d2_k + 1e-8) (see
    ured_interp_fwd in include/ured_hip.h). Differentiable in points1, points2 and d2 (whose
    gradient flows on into knn's backward and from there into both clouds); idx is not. The backward
    writes every gradient, sums in ascending (n,k) order: deterministic, no atomics."""

    @staticmethod
    def forward(ctx, points1, points2, idx, d2):
        who = "InterpFn"
        _lib.require_device(points1, points2, idx, d2)
        if idx.dim() != 3 or idx.dtype != torch.int32:
            raise ValueError(f"{who}: idx must be int32 [B,N,K], got {idx.dtype} {tuple(idx.shape)}")
        B, N, K = idx.shape
        if not 1 <= K <= MAX_K:
            raise ValueError(f"{who}: K {K} outside [1, {MAX_K}]")
        if d2.dtype != torch.float32 or tuple(d2.shape) != (B, N, K):
            raise ValueError(f"{who}: d2 must be float32 {(B, N, K)}, got {d2.dtype} {tuple(d2.shape)}")
        _, S = _cloud(who, "points2", points2, B, C=None)
        D2 = points2.shape[2]
        D1 = 0
        if points1 is not None:
            _, N1 = _cloud(who, "points1", points1, B, C=None)
            D1 = points1.shape[2]
            if N1 != N:
                raise ValueError(f"{who}: points1 has {N1} rows, idx {N}")
            if D1 < 1:
                raise ValueError(f"{who}: points1 has no channels")
        _same_device(who, points2, points1=points1, idx=idx, d2=d2)
        if N < 1 or S < 1 or D2 < 1:
            raise ValueError(f"{who}: N {N}, S {S} and D2 {D2} must be at least 1")
        if B > MAX_B:
            raise ValueError(f"{who}: B {B} exceeds {MAX_B}")
        if B * N * (D1 + D2) >= _LIM or B * S * D2 >= _LIM:
            raise ValueError(f"{who}: B * N * (D1 + D2) and B * S * D2 must stay below 2^31 "
                             f"(B={B} N={N} S={S} D1={D1} D2={D2})")
        p1 = None if points1 is None else points1.contiguous()
        p2, idx, d2 = points2.contiguous(), idx.contiguous(), d2.contiguous()
        out = torch.empty(B * N, D1 + D2, device=p2.device)
        w = torch.empty(B, N, K, device=p2.device)
        _lib.call("ured_interp_fwd", _lib.ptr(p2), _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(p1), B, N, S, K, D1, D2,
                  _lib.ptr(out), _lib.ptr(w), _lib.stream_of(p2))
        ctx.save_for_backward(p2, idx, w, d2)
        ctx.dims = (B, N, S, K, D1, D2)
        return out

    @staticmethod
    def backward(ctx, g):
        p2, idx, w, d2 = ctx.saved_tensors
        B, N, S, K, D1, D2 = ctx.dims
        g = g.contiguous()
        gp2 = torch.empty(B, S, D2, device=g.device)     # both written in full by the kernels
        gd2 = torch.empty(B, N, K, device=g.device)
        _lib.call("ured_interp_bwd", _lib.ptr(g), _lib.ptr(p2), _lib.ptr(idx), _lib.ptr(w), _lib.ptr(d2), B, N, S, K, D1,
                  D2, _lib.ptr(gp2), _lib.ptr(gd2), _lib.stream_of(g))
        need = ctx.needs_input_grad
        gp1 = g[:, :D1].view(B, N, D1) if D1 and need[0] else None      # the first D1 columns of g: a view
        return gp1, gp2 if need[1] else None, None, gd2 if need[3] else None
