"""3D-GCN graph convolution on the device (csrc/gcn.hip): the neighbour directions, the fused
Conv_surface / Conv_layer product-max-sum and Pool_layer's sampled max-pool of the reference's
network/P_3DGC.py, none of which builds a [B, V, n, S*C] tensor, and the layer's linear product on
the fp32 MFMA GEMM. Activations are point-major [B*V, C] fp32 rows, indices int32 and local to their
cloud; an index outside [0, V) reads as a zero row and takes no gradient. Every gradient is
deterministic (no float atomics). Arguments are validated before any device work. No CPU fallback."""
import ctypes

import torch
from torch.autograd import Function

from . import _lib
from . import kernels as K

GCN_NMAX = 255                    # URED_GCN_NMAX (include/ured_hip.h): the winning slot is a uint8
GCN_SMAX = 8                      # URED_GCN_SMAX: a lane keeps its 3 * S support components in registers
GCN_BWD_ROWS, GCN_BWD_PARTS = 16, 512   # URED_GCN_BWD_ROWS / _PARTS: the grad_sdn workspace's partial rows
MAX_B = 65535
_DGRAD_WGS, _DGRAD_SLICE = 64, 256    # GcnLinearFn's dgrad: workgroups aimed at, shortest slice of N per split
_LIM = 1 << 31

_P, _I, _SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
_lib.register({
    "ured_gcn_dirs": [_P, _P, _I, _I, _I, _P, _P],
    "ured_gcn_conv_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_gcn_conv_bwd_parts": [_I, _I],
    "ured_gcn_conv_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _SZ, _P],
    "ured_gcn_pool_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_gcn_pool_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
})


def bwd_parts(B, V):
    """Partial rows of GcnConvFn's grad_sdn workspace (ured_gcn_conv_bwd_parts)."""
    return max(1, min(-(-(B * V) // GCN_BWD_ROWS), GCN_BWD_PARTS))


def _f32(who, name, t, shape):
    """t must be a float32 tensor of `shape` (None entries are free)."""
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        want = "[" + ",".join("*" if s is None else str(s) for s in shape) + "]"
        raise ValueError(f"{who}: {name} must be {want}, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be float32, got {t.dtype}")


def _idx(who, name, idx):
    if idx.dim() != 3 or idx.dtype != torch.int32:
        raise ValueError(f"{who}: {name} must be int32 [B,V,n], got {idx.dtype} {tuple(idx.shape)}")
    return idx.shape


def _limits(who, B, V, n, S, C):
    if B > MAX_B:
        raise ValueError(f"{who}: B {B} exceeds {MAX_B}")
    if V < 1 or C < 1:
        raise ValueError(f"{who}: V {V} and C {C} must be at least 1")
    if not 1 <= n <= GCN_NMAX:
        raise ValueError(f"{who}: the neighbour count {n} is outside [1, {GCN_NMAX}] (the winning slot is a uint8)")
    if not 1 <= S <= GCN_SMAX:
        raise ValueError(f"{who}: the support count {S} is outside [1, {GCN_SMAX}]")
    if B * V * (S + 1) * C >= _LIM or B * V * n * 3 >= _LIM:
        raise ValueError(f"{who}: B * V * (S + 1) * C and B * V * n * 3 must stay below 2^31 "
                         f"(B={B} V={V} n={n} S={S} C={C})")


def _same_device(who, ref, **others):
    for name, t in others.items():
        if t is not None and t.device != ref.device:
            raise ValueError(f"{who}: {name} is on {t.device}, expected {ref.device}")


def neighbor_dirs(vertices, idx):
    """vertices [B,V,3] fp32, idx int32 [B,V,n] -> [B,V,n,3]: (vertices[idx] - vertices[v]) /
    max(|.|, 1e-12), the reference's get_neighbor_direction_norm; a coincident neighbour gives the
    zero vector. vertices is data: a tensor that requires grad is refused."""
    who = "neighbor_dirs"
    _f32(who, "vertices", vertices, (None, None, 3))
    B, V, n = _idx(who, "idx", idx)
    if tuple(vertices.shape[:2]) != (B, V):
        raise ValueError(f"{who}: idx {tuple(idx.shape)} does not match vertices {tuple(vertices.shape)}")
    if vertices.requires_grad:
        raise ValueError(f"{who}: vertices requires grad, but the directions are computed as data (no gradient "
                         "flows to the vertex coordinates); detach it")
    _limits(who, B, V, n, 1, 1)
    _lib.require_device(vertices, idx)
    _same_device(who, vertices, idx=idx)
    vertices, idx = vertices.contiguous(), idx.contiguous()
    out = torch.empty(B, V, n, 3, device=vertices.device)
    _lib.call("ured_gcn_dirs", _lib.ptr(vertices), _lib.ptr(idx), B, V, n, _lib.ptr(out), _lib.stream_of(vertices))
    return out


def _conv_check(who, dirn, sdn, feat, idx, S):
    B, V, n = _idx(who, "idx", idx)
    if dirn.dim() != 4 or dirn.shape[-1] != 3:
        raise ValueError(f"{who}: dirn must be [B,V,n,3], got {tuple(dirn.shape)}")
    if tuple(dirn.shape[:3]) != (B, V, n):
        raise ValueError(f"{who}: idx {tuple(idx.shape)} does not match dirn {tuple(dirn.shape)}")
    _f32(who, "dirn", dirn, (B, V, n, 3))
    _f32(who, "sdn", sdn, (3, None))
    S = int(S)
    if not 1 <= S <= GCN_SMAX:
        raise ValueError(f"{who}: the support count {S} is outside [1, {GCN_SMAX}]")
    C = sdn.shape[1] // S
    if C < 1 or C * S != sdn.shape[1]:
        raise ValueError(f"{who}: sdn has {sdn.shape[1]} columns, not S * C with S = {S}")
    if feat is not None:
        _f32(who, "feat", feat, (B * V, (S + 1) * C))
    _limits(who, B, V, n, S, C)
    if dirn.requires_grad:
        raise ValueError(f"{who}: dirn requires grad, but the directions are data")
    return B, V, n, S, C


class GcnConvFn(Function):
    """(dirn [B,V,n,3], sdn [3, S*C], feat [B*V, (S+1)*C] | None, idx int32 [B,V,n], S) ->
    (out [B*V, C], slot uint8 [B*V, S, C]).
    With feat (Conv_layer): out[b,v,c] = feat[b,v,c] + sum_s max_j relu(dirn[b,v,j,:] . sdn[:, s*C+c])
    * feat[b, idx[b,v,j], C + s*C + c]; without (Conv_surface): sum_s max_j relu(.). slot is the
    winning j, the lowest on a tie (a tie at 0 carries no gradient under any winner); relu passes a
    gradient iff theta > 0. Differentiable in sdn and feat; dirn and idx are data, slot is not
    differentiable. Both gradients are fixed-order sums, bitwise equal from run to run."""

    @staticmethod
    def forward(ctx, dirn, sdn, feat, idx, S):
        who = "GcnConvFn"
        B, V, n, S, C = _conv_check(who, dirn, sdn, feat, idx, S)
        _lib.require_device(dirn, sdn, feat, idx)
        _same_device(who, dirn, sdn=sdn, feat=feat, idx=idx)
        dirn, sdn, idx = dirn.contiguous(), sdn.contiguous(), idx.contiguous()
        feat = None if feat is None else feat.contiguous()
        dev = dirn.device
        out = torch.empty(B * V, C, device=dev)
        slot = torch.empty(B * V, S, C, dtype=torch.uint8, device=dev)
        _lib.call("ured_gcn_conv_fwd", _lib.ptr(dirn), _lib.ptr(sdn), _lib.ptr(feat), _lib.ptr(idx), B, V, n, S, C,
                  _lib.ptr(out), _lib.ptr(slot), _lib.stream_of(dirn))
        ctx.save_for_backward(dirn, sdn, feat, idx, slot)
        ctx.dims = (B, V, n, S, C)
        ctx.mark_non_differentiable(slot)
        return out, slot

    @staticmethod
    def backward(ctx, g, _gslot):
        dirn, sdn, feat, idx, slot = ctx.saved_tensors
        B, V, n, S, C = ctx.dims
        g = g.contiguous()
        dev = g.device
        gfeat = None if feat is None else torch.empty(B * V, (S + 1) * C, device=dev)   # written in full, as gsdn
        gsdn = torch.empty(3, S * C, device=dev)
        ws = torch.empty(bwd_parts(B, V) * 3 * S * C, device=dev)
        _lib.call("ured_gcn_conv_bwd", _lib.ptr(g), _lib.ptr(dirn), _lib.ptr(sdn), _lib.ptr(feat), _lib.ptr(idx),
                  _lib.ptr(slot), B, V, n, S, C, _lib.ptr(gfeat), _lib.ptr(gsdn), _lib.ptr(ws), ws.numel(),
                  _lib.stream_of(g))
        need = ctx.needs_input_grad
        return None, gsdn if need[1] else None, gfeat if need[2] else None, None, None


def _pool_check(who, feat, idx, sample):
    B, V, k = _idx(who, "idx", idx)
    _f32(who, "feat", feat, (B * V, None))
    C = feat.shape[1]
    if sample.dim() != 1 or sample.dtype != torch.int32:
        raise ValueError(f"{who}: sample must be int32 [P], got {sample.dtype} {tuple(sample.shape)}")
    P = sample.shape[0]
    if B > MAX_B:
        raise ValueError(f"{who}: B {B} exceeds {MAX_B}")
    if V < 1 or C < 1:
        raise ValueError(f"{who}: V {V} and C {C} must be at least 1")
    if not 1 <= k <= GCN_NMAX:
        raise ValueError(f"{who}: the neighbour count {k} is outside [1, {GCN_NMAX}] (the winning slot is a uint8)")
    if max(B * V * C, B * P * C, B * V * k, P * k) >= _LIM:
        raise ValueError(f"{who}: B * V * C, B * P * C, B * V * k and P * k must stay below 2^31 "
                         f"(B={B} V={V} P={P} k={k} C={C})")
    return B, V, k, P, C


class GcnPoolFn(Function):
    """(feat [B*V, C], idx int32 [B,V,k], sample int32 [P]) -> (out [B*P, C], slot uint8 [B*P, C]):
    out[b,p,c] = max_j feat[b, idx[b, sample[p], j], c] for the sampled vertices only (the reference's
    Pool_layer pools every vertex and then keeps these); slot is the winning j, the lowest on a tie.
    The backward scatters grad_out to the winning rows in ascending (p, j) order: no atomics."""

    @staticmethod
    def forward(ctx, feat, idx, sample):
        who = "GcnPoolFn"
        B, V, k, P, C = _pool_check(who, feat, idx, sample)
        _lib.require_device(feat, idx, sample)
        _same_device(who, feat, idx=idx, sample=sample)
        feat, idx, sample = feat.contiguous(), idx.contiguous(), sample.contiguous()
        out = torch.empty(B * P, C, device=feat.device)
        slot = torch.empty(B * P, C, dtype=torch.uint8, device=feat.device)
        _lib.call("ured_gcn_pool_fwd", _lib.ptr(feat), _lib.ptr(idx), _lib.ptr(sample), B, V, k, P, C, _lib.ptr(out),
                  _lib.ptr(slot), _lib.stream_of(feat))
        ctx.save_for_backward(idx, sample, slot)
        ctx.dims = (B, V, k, P, C)
        ctx.mark_non_differentiable(slot)
        return out, slot

    @staticmethod
    def backward(ctx, g, _gslot):
        idx, sample, slot = ctx.saved_tensors
        B, V, k, P, C = ctx.dims
        g = g.contiguous()
        gfeat = torch.empty(B * V, C, device=g.device)       # written in full by the kernel
        _lib.call("ured_gcn_pool_bwd", _lib.ptr(g), _lib.ptr(idx), _lib.ptr(sample), _lib.ptr(slot), B, V, k, P, C,
                  _lib.ptr(gfeat), _lib.stream_of(g))
        return gfeat, None, None


class GcnLinearFn(Function):
    """x [M, K] @ weights [K, N] + bias [N] -> [M, N] (Conv_layer's feature_map @ weights + bias) on the
    fp32 MFMA GEMM: the store epilogue with bias forward, the b_kmajor dgrad, the split-K wgrad and
    the column sums for the bias. The GEMM reads weights as [N][K] rows, so the (small) matrix is
    transposed once per call and its gradient transposed back."""

    @staticmethod
    def forward(ctx, x, weights, bias):
        who = "GcnLinearFn"
        _f32(who, "x", x, (None, None))
        M, Kd = x.shape
        _f32(who, "weights", weights, (Kd, None))
        N = weights.shape[1]
        _f32(who, "bias", bias, (N,))
        if M < 1 or Kd < 1 or N < 1:
            raise ValueError(f"{who}: empty operand (M={M} K={Kd} N={N})")
        if M * max(Kd, N) >= _LIM:
            raise ValueError(f"{who}: M * max(K, N) must stay below 2^31 (M={M} K={Kd} N={N})")
        _lib.require_device(x, weights, bias)
        _same_device(who, x, weights=weights, bias=bias)
        x, bias = x.contiguous(), bias.contiguous()
        wt = weights.t().contiguous()                        # [N][K]
        y = torch.empty(M, N, device=x.device)
        K.gemm(M, N, Kd, x, Kd, wt, Kd, y, N, bias=bias)
        ctx.save_for_backward(x, wt)
        return y

    @staticmethod
    def backward(ctx, g):
        x, wt = ctx.saved_tensors
        M, Kd = x.shape
        N = wt.shape[0]
        g = g.contiguous()
        need = ctx.needs_input_grad
        dx = dw = db = None
        if need[0]:
            dx = torch.empty(M, Kd, device=g.device)
            # K.gemm's own split of a few-tile store GEMM takes up to 1024 / tiles slices of the long
            # N: a workspace several times the layer's activations (16.8 MB at M 1024, K 128, N 1024).
            # At most 64 / tiles slices of at least 256 keep it near the activations' own size.
            tiles = K.nblocks(M) * K.nblocks(Kd)
            if tiles > 16:                                   # enough tiles: K.gemm stores in one pass
                K.gemm(M, Kd, N, g, N, wt, Kd, dx, Kd, b_kmajor=True)
            else:
                sp = max(1, min(_DGRAD_WGS // tiles, N // _DGRAD_SLICE))
                ws = torch.empty(sp, M, Kd, device=g.device) if sp > 1 else dx
                K.gemm(M, Kd, N, g, N, wt, Kd, ws, Kd, b_kmajor=True, epi=K.EPI_SPLITK, splits=sp)
                if sp > 1:
                    K.splitk_reduce(ws, sp, M, Kd, dx, Kd)
        if need[1]:
            dwt = torch.empty(N, Kd, device=g.device)
            K.wgrad(g, N, x, Kd, N, Kd, M, dwt, Kd)
            dw = dwt.t()
        if need[2]:
            db = K.colsum(g)
        return dx, dw, db
