"""Vector-Neuron DGCNN layers on the device (csrc/vn.hip): the feature-space kNN, the fused
get_graph_feature + VNLinearLeakyReLU edge layer (VnEdgeFn), its per-point form (VnPointFn),
VNMaxPool (VnMaxPoolFn) and VNStdFeature's frame product (VnFrameFn) of the reference's network/VN/.
A VN feature is point-major with the channel innermost, [B, N, 3, C] fp32, so x.view(B*N*3, C) is an
operand of the fp32 MFMA GEMM; indices are int32 and local to their cloud. The linear maps of an edge
layer act on [x_j - x_i, x_i], so W . edge = W_a x_j + (W_b - W_a) x_i: two per-point products (one
GEMM) instead of a per-edge one, and everything after them is evaluated per edge in registers. With
pool="mean" no [B, N, k, ., C] float tensor exists in the forward; the backward uses one per-edge
workspace, freed on return. Every gradient is deterministic (no float atomics). Arguments are
validated before any device work. No CPU fallback."""
import ctypes

import torch
from torch.autograd import Function

from . import _lib
from . import kernels as K

VN_KMAX = 32                      # URED_VN_KMAX (include/ured_hip.h)
VN_DMAX = 256                     # URED_VN_DMAX
VN_COMAX = 384                    # URED_VN_COMAX
VN_STAT_ROWS, VN_PARTS = 16, 256  # URED_VN_STAT_ROWS / _PARTS: the BatchNorm workspaces' partial rows
MAX_B = 65535
_LIM = 1 << 31

_P, _I, _SZ, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
_lib.register({
    "ured_vn_parts": [_I, _I],
    "ured_vn_knn": [_P, _I, _I, _I, _I, _P, _P, _SZ, _P],
    "ured_vn_act_fwd": [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _F, _F, _I, _P, _SZ, _P, _P, _P, _P],
    "ured_vn_act_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _SZ, _P, _P, _SZ, _P, _P, _P, _P],
    "ured_vn_maxpool_fwd": [_P, _P, _I, _I, _I, _I, _P, _P, _P],
    "ured_vn_maxpool_bwd": [_P, _P, _I, _I, _I, _I, _P, _P],
    "ured_vn_frame_fwd": [_P, _P, _I, _I, _P, _P],
    "ured_vn_frame_bwd": [_P, _P, _P, _I, _I, _P, _P, _P],
})


def stat_parts(B, N):
    """Partial rows of the BatchNorm workspaces (ured_vn_parts)."""
    return max(1, min(-(-(B * N) // VN_STAT_ROWS), VN_PARTS))


def _f32(who, name, t, shape):
    """t must be a float32 tensor of `shape` (None entries are free)."""
    if not torch.is_tensor(t) or t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        want = "[" + ",".join("*" if s is None else str(s) for s in shape) + "]"
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{who}: {name} must be {want}, got {got}")
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")


def _same_device(who, ref, **others):
    for name, t in others.items():
        if t is not None and t.device != ref.device:
            raise ValueError(f"{who}: {name} is on {t.device}, expected {ref.device}")


def knn_rows(x, K_):
    """x [B,N,D] fp32 -> idx int32 [B,N,K]: the K rows of the same cloud nearest to each row, the row
    itself included, ranked by (distance, index) with the lowest index first on a tie; the distance is
    the direct squared difference summed over ascending d. No gradient."""
    who = "knn_rows"
    _f32(who, "x", x, (None, None, None))
    B, N, D = x.shape
    K_ = int(K_)
    if B > MAX_B:
        raise ValueError(f"{who}: B {B} exceeds {MAX_B}")
    if N < 1 or not 1 <= D <= VN_DMAX:
        raise ValueError(f"{who}: N {N} must be at least 1 and D {D} within [1, {VN_DMAX}]")
    if not 1 <= K_ <= VN_KMAX:
        raise ValueError(f"{who}: K {K_} is outside [1, {VN_KMAX}]")
    if K_ > N:
        raise ValueError(f"{who}: K {K_} exceeds the cloud's {N} points")
    if B * N * max(D, K_) >= _LIM:
        raise ValueError(f"{who}: B * N * max(D, K) must stay below 2^31 (B={B} N={N} D={D} K={K_})")
    _lib.require_device(x)
    x = x.detach().contiguous()
    idx = torch.empty(B, N, K_, dtype=torch.int32, device=x.device)
    ws = torch.empty(B * N * N, device=x.device)              # the clouds' distance matrices, freed on return
    _lib.call("ured_vn_knn", _lib.ptr(x), B, N, D, K_, _lib.ptr(idx), _lib.ptr(ws), ws.numel(), _lib.stream_of(x))
    return idx


def _bn_check(who, bn, Co):
    for name in ("running_mean", "running_var", "num_batches_tracked", "momentum", "eps", "training"):
        if not hasattr(bn, name):
            raise ValueError(f"{who}: bn must be a BatchNorm module (no attribute {name})")
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError(f"{who}: bn must track running statistics")
    if bn.momentum is None:
        raise ValueError(f"{who}: bn.momentum = None (a cumulative average) is not supported")
    _f32(who, "bn.running_mean", bn.running_mean, (Co,))
    _f32(who, "bn.running_var", bn.running_var, (Co,))


def _act_check(who, x, idx, Wf, Wd, gamma, beta, bn, pool):
    """-> (B, N, k, C, Co, Cd, edge, pool_mean)."""
    _f32(who, "x", x, (None, None, 3, None))
    B, N, _, C = x.shape
    edge = idx is not None
    k = 1
    if edge:
        if idx.dim() != 3 or idx.dtype != torch.int32 or tuple(idx.shape[:2]) != (B, N):
            raise ValueError(f"{who}: idx must be int32 [B,N,k] = [{B},{N},k], got {idx.dtype} {tuple(idx.shape)}")
        k = idx.shape[2]
    if pool not in ("mean", "none"):
        raise ValueError(f"{who}: pool must be 'mean' or 'none', got {pool!r}")
    Kin = 2 * C if edge else C
    _f32(who, "Wf", Wf, (None, Kin))
    Co = Wf.shape[0]
    _f32(who, "Wd", Wd, (None, Kin))
    Cd = Wd.shape[0]
    if Cd not in (1, Co):
        raise ValueError(f"{who}: Wd has {Cd} rows, not Co = {Co} (per channel) or 1 (shared)")
    _f32(who, "gamma", gamma, (Co,))
    _f32(who, "beta", beta, (Co,))
    _bn_check(who, bn, Co)
    if B > MAX_B:
        raise ValueError(f"{who}: B {B} exceeds {MAX_B}")
    if N < 1 or C < 1:
        raise ValueError(f"{who}: N {N} and C {C} must be at least 1")
    if not 1 <= k <= VN_KMAX:
        raise ValueError(f"{who}: the neighbour count {k} is outside [1, {VN_KMAX}]")
    if not 1 <= Co <= VN_COMAX:
        raise ValueError(f"{who}: Co {Co} is outside [1, {VN_COMAX}]")
    if B * N * k * 6 * (Co + Cd) >= _LIM or B * N * 3 * C >= _LIM:
        raise ValueError(f"{who}: B * N * k * 6 * (Co + Cd) and B * N * 3 * C must stay below 2^31 "
                         f"(B={B} N={N} k={k} C={C} Co={Co} Cd={Cd})")
    if bn.training and B * N * k <= 1:
        raise ValueError(f"{who}: batch statistics need more than one value per channel (B * N * k = {B * N * k})")
    return B, N, k, C, Co, Cd, edge, pool == "mean"


def _act_forward(ctx, who, x, idx, Wf, Wd, gamma, beta, bn, pool):
    B, N, k, C, Co, Cd, edge, pool_mean = _act_check(who, x, idx, Wf, Wd, gamma, beta, bn, pool)
    _lib.require_device(x, idx, Wf, Wd, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    _same_device(who, x, idx=idx, Wf=Wf, Wd=Wd, gamma=gamma, beta=beta, running_mean=bn.running_mean,
                 running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked)
    dev = x.device
    x = x.contiguous()
    idx = None if idx is None else idx.contiguous()
    gamma, beta = gamma.contiguous(), beta.contiguous()
    if edge:                                                 # [Wf_a; Wd_a; Wf_b - Wf_a; Wd_b - Wd_a]
        wcat = torch.cat((Wf[:, :C], Wd[:, :C], Wf[:, C:] - Wf[:, :C], Wd[:, C:] - Wd[:, :C]), 0).contiguous()
    else:
        wcat = torch.cat((Wf, Wd), 0).contiguous()
    LD = wcat.shape[0]
    M = B * N * 3
    training = bool(bn.training)
    uv = torch.empty(M, LD, device=dev)
    out = torch.empty((B, N, 3, Co) if pool_mean else (B, N, k, 3, Co), device=dev)
    mask = torch.empty(B, N, k, Co, dtype=torch.uint8, device=dev)
    stat = torch.empty(4, Co, device=dev)
    if B > 0:
        K.gemm(M, LD, C, x, C, wcat, C, uv, LD)
    ws = torch.empty(stat_parts(B, N) * 2 * Co, dtype=torch.float64, device=dev) if training else None
    _lib.call("ured_vn_act_fwd", _lib.ptr(uv), _lib.ptr(idx), B, N, k, Co, Cd, int(training), _lib.ptr(gamma), _lib.ptr(beta),
              _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), _lib.ptr(bn.num_batches_tracked), float(bn.momentum),
              float(bn.eps), int(pool_mean), _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.ptr(stat), _lib.ptr(out),
              _lib.ptr(mask), _lib.stream_of(x))
    ctx.save_for_backward(x, idx, wcat, uv, mask, stat)
    ctx.dims = (B, N, k, C, Co, Cd, edge, pool_mean, training)
    ctx.mark_non_differentiable(mask)
    return out, mask


def _act_backward(ctx, g, need_x, need_w):
    """-> (grad_x, grad_Wf, grad_Wd, grad_gamma, grad_beta); the GEMM for grad_x and the weight-gradient
    GEMM run only where asked for."""
    x, idx, wcat, uv, mask, stat = ctx.saved_tensors
    B, N, k, C, Co, Cd, edge, pool_mean, training = ctx.dims
    dev = g.device
    g = g.contiguous()
    W = Co + Cd
    LD = wcat.shape[0]
    M = B * N * 3
    guv = torch.empty(M, LD, device=dev)                     # written in full by the kernels, as the rest
    ggamma, gbeta = torch.empty(Co, device=dev), torch.empty(Co, device=dev)
    coef = torch.empty(2, Co, device=dev)
    ws = torch.empty(stat_parts(B, N) * 2 * Co, dtype=torch.float64, device=dev)
    edge_ws = torch.empty(B * N * k * 3 * W, device=dev) if edge else None
    _lib.call("ured_vn_act_bwd", _lib.ptr(g), _lib.ptr(uv), _lib.ptr(idx), _lib.ptr(mask), B, N, k, Co, Cd, int(training),
              int(pool_mean), _lib.ptr(stat), _lib.ptr(ws), ws.numel(), _lib.ptr(coef), _lib.ptr(edge_ws),
              0 if edge_ws is None else edge_ws.numel(), _lib.ptr(guv), _lib.ptr(ggamma), _lib.ptr(gbeta), _lib.stream_of(g))
    del edge_ws
    gx = gWf = gWd = None
    if need_x:
        gx = torch.empty(B, N, 3, C, device=dev)
        if B > 0:
            K.gemm(M, C, LD, guv, LD, wcat, C, gx, C, b_kmajor=True)
    if not need_w:
        return gx, gWf, gWd, ggamma, gbeta
    gw = torch.empty(LD, C, device=dev)
    if B > 0:
        K.wgrad(guv, LD, x, C, LD, C, M, gw, C)
    else:
        gw.zero_()
    if edge:
        guf, gud, gvf, gvd = gw[:Co], gw[Co:W], gw[W:W + Co], gw[W + Co:]
        gWf, gWd = torch.cat((guf - gvf, gvf), 1), torch.cat((gud - gvd, gvd), 1)
    else:
        gWf, gWd = gw[:Co], gw[Co:]
    return gx, gWf, gWd, ggamma, gbeta


class VnEdgeFn(Function):
    """(x [B,N,3,C], idx int32 [B,N,k], Wf [Co,2C], Wd [Co or 1, 2C], gamma [Co], beta [Co], bn, pool) ->
    (out, mask): get_graph_feature + VNLinearLeakyReLU(dim=5). Per edge (b,n,j), p and d are
    U[idx[b,n,j]] + V[n] with U = x W_a^T, V = x (W_b - W_a)^T on the GEMM (W_a the first C columns);
    nrm = |p| + 1e-6, ph = p / nrm * bn(nrm) with the BatchNorm over all B*N*k edges per channel,
    out = ph where <ph,d> >= 0 and 0.2 ph + 0.8 (ph - <ph,d> / (|d|^2 + 1e-6) d) elsewhere. bn is the
    nn.BatchNorm2d that owns gamma / beta: its mode, momentum, eps and running buffers are used and,
    in training, updated as nn.BatchNorm2d does. pool = "mean": out [B,N,3,Co], the mean over j;
    "none": out [B,N,k,3,Co]. mask uint8 [B,N,k,Co] is the branch taken (1: <ph,d> >= 0), saved for
    the backward. Differentiable in x, Wf, Wd, gamma, beta; idx is data."""

    @staticmethod
    def forward(ctx, x, idx, Wf, Wd, gamma, beta, bn, pool):
        if idx is None:
            raise ValueError("VnEdgeFn: idx is required (VnPointFn is the form without a gather)")
        return _act_forward(ctx, "VnEdgeFn", x, idx, Wf, Wd, gamma, beta, bn, pool)

    @staticmethod
    def backward(ctx, g, _gmask):
        need = ctx.needs_input_grad
        gx, gWf, gWd, gg, gb = _act_backward(ctx, g, need[0], need[2] or need[3])
        return (gx if need[0] else None, None, gWf if need[2] else None, gWd if need[3] else None,
                gg if need[4] else None, gb if need[5] else None, None, None)


class VnPointFn(Function):
    """(x [B,N,3,C], Wf [Co,C], Wd [Co or 1, C], gamma, beta, bn) -> (out [B,N,3,Co], mask uint8 [B,N,Co]):
    VNLinearLeakyReLU(dim=4), the same normalise + leaky pair without a gather; the BatchNorm (an
    nn.BatchNorm1d) runs over the B*N points per channel."""

    @staticmethod
    def forward(ctx, x, Wf, Wd, gamma, beta, bn):
        out, mask = _act_forward(ctx, "VnPointFn", x, None, Wf, Wd, gamma, beta, bn, "mean")
        return out, mask.view(mask.shape[0], mask.shape[1], mask.shape[3])

    @staticmethod
    def backward(ctx, g, _gmask):
        need = ctx.needs_input_grad
        gx, gWf, gWd, gg, gb = _act_backward(ctx, g, need[0], need[1] or need[2])
        return (gx if need[0] else None, gWf if need[1] else None, gWd if need[2] else None, gg if need[3] else None,
                gb if need[4] else None, None)


def vn_edge(x, idx, Wf, Wd, bn, pool="mean"):
    """VnEdgeFn with bn's own affine parameters."""
    return VnEdgeFn.apply(x, idx, Wf, Wd, bn.weight, bn.bias, bn, pool)


def vn_point(x, Wf, Wd, bn):
    """VnPointFn with bn's own affine parameters."""
    return VnPointFn.apply(x, Wf, Wd, bn.weight, bn.bias, bn)


class VnMaxPoolFn(Function):
    """(x_edge [B,N,k,3,C], Wp [C,C]) -> (out [B,N,3,C], slot uint8 [B,N,C]): VNMaxPool. d = Wp . x on
    the GEMM; the winner over j is the largest <x,d>, the lowest j on a tie; out is the winning edge's
    vector. The gradient goes to the winning edge only; Wp gets none, as in the reference."""

    @staticmethod
    def forward(ctx, x, Wp):
        who = "VnMaxPoolFn"
        _f32(who, "x_edge", x, (None, None, None, 3, None))
        B, N, k, _, C = x.shape
        _f32(who, "Wp", Wp, (C, C))
        if B > MAX_B:
            raise ValueError(f"{who}: B {B} exceeds {MAX_B}")
        if N < 1 or C < 1:
            raise ValueError(f"{who}: N {N} and C {C} must be at least 1")
        if not 1 <= k <= VN_KMAX:
            raise ValueError(f"{who}: the neighbour count {k} is outside [1, {VN_KMAX}]")
        if B * N * k * 3 * C >= _LIM:
            raise ValueError(f"{who}: B * N * k * 3 * C must stay below 2^31 (B={B} N={N} k={k} C={C})")
        _lib.require_device(x, Wp)
        _same_device(who, x, Wp=Wp)
        x, Wp = x.contiguous(), Wp.detach().contiguous()
        dev = x.device
        M = B * N * k * 3
        d = torch.empty(M, C, device=dev)
        if B > 0:
            K.gemm(M, C, C, x, C, Wp, C, d, C)
        out = torch.empty(B, N, 3, C, device=dev)
        slot = torch.empty(B, N, C, dtype=torch.uint8, device=dev)
        _lib.call("ured_vn_maxpool_fwd", _lib.ptr(x), _lib.ptr(d), B, N, k, C, _lib.ptr(out), _lib.ptr(slot),
                  _lib.stream_of(x))
        ctx.save_for_backward(slot)
        ctx.dims = (B, N, k, C)
        ctx.mark_non_differentiable(slot)
        return out, slot

    @staticmethod
    def backward(ctx, g, _gslot):
        slot, = ctx.saved_tensors
        B, N, k, C = ctx.dims
        g = g.contiguous()
        gx = torch.empty(B, N, k, 3, C, device=g.device)     # written in full by the kernel
        _lib.call("ured_vn_maxpool_bwd", _lib.ptr(g), _lib.ptr(slot), B, N, k, C, _lib.ptr(gx), _lib.stream_of(g))
        return gx, None


class VnFrameFn(Function):
    """(x [B,N,3,C], z [B,N,3,3]) -> out [B,N,3,C], out[b,n,k,c] = sum_j x[b,n,j,c] z[b,n,j,k]:
    the einsum('bijm,bjkm->bikm') of VNStdFeature in the point-major layout. Differentiable in both."""

    @staticmethod
    def forward(ctx, x, z):
        who = "VnFrameFn"
        _f32(who, "x", x, (None, None, 3, None))
        B, N, _, C = x.shape
        _f32(who, "z", z, (B, N, 3, 3))
        if C < 1 or B * N * 3 * C >= _LIM:
            raise ValueError(f"{who}: C must be at least 1 and B * N * 3 * C below 2^31 (B={B} N={N} C={C})")
        _lib.require_device(x, z)
        _same_device(who, x, z=z)
        x, z = x.contiguous(), z.contiguous()
        out = torch.empty(B, N, 3, C, device=x.device)
        _lib.call("ured_vn_frame_fwd", _lib.ptr(x), _lib.ptr(z), B * N, C, _lib.ptr(out), _lib.stream_of(x))
        ctx.save_for_backward(x, z)
        return out

    @staticmethod
    def backward(ctx, g):
        x, z = ctx.saved_tensors
        B, N, _, C = x.shape
        g = g.contiguous()
        gx, gz = torch.empty_like(x), torch.empty_like(z)     # written in full by the kernel
        _lib.call("ured_vn_frame_bwd", _lib.ptr(g), _lib.ptr(x), _lib.ptr(z), B * N, C, _lib.ptr(gx), _lib.ptr(gz),
                  _lib.stream_of(g))
        need = ctx.needs_input_grad
        return gx if need[0] else None, gz if need[1] else None


class VnLinearFn(Function):
    """x [M, K] @ W [N, K]^T -> [M, N] on the fp32 MFMA GEMM (a bias-free nn.Linear on rows)."""

    @staticmethod
    def forward(ctx, x, W):
        who = "VnLinearFn"
        _f32(who, "x", x, (None, None))
        M, Kd = x.shape
        _f32(who, "W", W, (None, Kd))
        N = W.shape[0]
        if M < 1 or Kd < 1 or N < 1 or M * max(Kd, N) >= _LIM:
            raise ValueError(f"{who}: sizes must be at least 1 and M * max(K, N) below 2^31 (M={M} K={Kd} N={N})")
        _lib.require_device(x, W)
        _same_device(who, x, W=W)
        x, W = x.contiguous(), W.contiguous()
        y = torch.empty(M, N, device=x.device)
        K.gemm(M, N, Kd, x, Kd, W, Kd, y, N)
        ctx.save_for_backward(x, W)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        M, Kd = x.shape
        N = W.shape[0]
        g = g.contiguous()
        need = ctx.needs_input_grad
        dx = dw = None
        if need[0]:
            dx = torch.empty(M, Kd, device=g.device)
            K.gemm(M, Kd, N, g, N, W, Kd, dx, Kd, b_kmajor=True)
        if need[1]:
            dw = torch.empty(N, Kd, device=g.device)
            K.wgrad(g, N, x, Kd, N, Kd, M, dw, Kd)
        return dx, dw
