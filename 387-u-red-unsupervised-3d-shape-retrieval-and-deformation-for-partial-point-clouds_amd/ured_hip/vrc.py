"""VRCNet's self-attention encoder (Density_aware_Chamfer_Distance/models/vrcnet.py:15-290) as autograd
Functions on libured_hip.so: every matrix product is ured_gemm (ured_hip.kernels), the rest the kernels
of csrc/vrc.hip. Activations are point-major [B*N][C] fp32; the contracts are written out in
include/ured_hip.h.

SaFn        the attention core of SA_module on the projected rows P = [x1 | x2p | x3p]: the 1x1
            convolutions commute with the neighbour gather, so they run once per point (one GEMM) and
            the kernel gathers rows; no [B, C, k, N] tensor exists. Saved for the backward: P, idx, o
            and the per-point h [ms] and w [k ms].
SkMeanFn    s[b][c] = mean over points of sum_i relu(y_i): the input of SK_SA_module's fc.
SkMixFn     relu?(sum_i a[b][i][c] relu(y_i)): the selected feature.
EdgePoolFn  centre row | max over the pk neighbour rows (lowest j on a tie), with the winning slot.
UnpoolFn    three-point interpolation with given weights | skip features.
EfEdgeFn    the per-edge rows of EF_expansion, relu((G +) centre[n] + neighbour[idx[n, j]]) from the per-point
            halves of conv1 / conv2; no [B, 2C, k, N] or [B, O + 2C, k, N] tensor exists.
EfMaxFn     the max over the k slots of conv3's rows (lowest j on a tie), with the winning slot.
FoldFn      relu(U[n] + T[s]) over the r grid points of every coarse point (Folding).
LatentFn    Model's latent heads: softplus, the reparameterised samples stacked as the generator's [2B, Z]
            input, KL(N(0,1) || prior) and KL(prior || posterior); one launch each way, nothing saved but the inputs.
GaussKernelFn  compute_kernel's exp(-mean_d((x_i - y_j)^2) / Z) without the two [n, m, Z] tiled tensors.
LinearRowsFn / ReluFn / MaxRowsFn  the GEMM layers between them (bias, ReLU prologue, per-cloud row
            bias), the ReLU and the max over a cloud's points.
Arguments are validated before any device work; a tensor off the device raises (no CPU path).
Backwards write every element, sum in a fixed ascending order and use no atomics. Caller's stream.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _lib
from . import kernels as K
from .pcn import _Relu, center_bwd, center_fwd, pool_bwd, relu

_P, _I = ctypes.c_void_p, ctypes.c_int
_lib.register({
    "ured_vrc_sa_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "ured_vrc_sa_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "ured_vrc_sk_mean_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    "ured_vrc_sk_mean_bwd": [_P, _P, _I, _I, _I, _P, _P],
    "ured_vrc_sk_mix_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    "ured_vrc_sk_mix_bwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "ured_vrc_pool_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_vrc_pool_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    "ured_vrc_unpool_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P],
    "ured_vrc_unpool_bwd": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_vrc_ef_edge_fwd": [_P, _P, _P, _I, _I, _I, _I, _P, _P],
    "ured_vrc_ef_edge_bwd": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "ured_vrc_ef_max_fwd": [_P, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_vrc_ef_max_bwd": [_P, _P, _I, _I, _I, _I, _I, _P, _P],
    "ured_vrc_fold_fwd": [_P, _P, _I, _I, _I, _I, _P, _P],
    "ured_vrc_fold_bwd": [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_vrc_latent_fwd": [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P],
    "ured_vrc_latent_bwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P],
    "ured_vrc_gauss_fwd": [_P, _P, _I, _I, _I, _P, _P],
    "ured_vrc_gauss_bwd": [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
})

KMAX, RELMAX, MIDMAX, MSMAX, MMAX, PKMAX = 32, 32, 128, 16, 4, 32      # URED_VRC_* (include/ured_hip.h)
CMAX = 512                          # URED_VRC_CMAX: the widest SA_module / EF_expansion input
OMAX, RMAX = 256, 16                # URED_VRC_OMAX, URED_VRC_RMAX: EF_expansion's output_size and step_ratio
ZMAX, GAUSS_MAX = 4096, 4096         # URED_VRC_ZMAX, URED_VRC_GAUSS_MAX: the latent width, the rows of a Gaussian kernel
MAX_B = 65535
_LIM = 1 << 31
WA_MIN_CHUNK, WA_CHUNKS = 32, 1024  # points per workgroup of the dWa partials: at least 32, about 1024 workgroups
FOLD_MIN_CHUNK, FOLD_CHUNKS = 32, 256   # the same for the dT partials of FoldFn


def _p(t):
    return None if t is None else t.data_ptr()


def _f32(who, name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be a float32 tensor")
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {shape}")


def _i32(who, name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.int32:
        raise TypeError(f"{who}: {name} must be an int32 tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {shape}")


def sa_check(who, B, N, k, rel, mid, share_planes):
    """The limits of the attention core -> ms."""
    if not 1 <= k <= KMAX:
        raise ValueError(f"{who}: k {k} outside [1, {KMAX}]")
    if k > N:
        raise ValueError(f"{who}: k {k} exceeds the cloud's {N} points")
    if not 1 <= rel <= RELMAX or not 1 <= mid <= MIDMAX:
        raise ValueError(f"{who}: rel {rel} outside [1, {RELMAX}] or mid {mid} outside [1, {MIDMAX}]")
    if share_planes < 1 or mid % share_planes:
        raise ValueError(f"{who}: share_planes {share_planes} must divide mid {mid}")
    ms = mid // share_planes
    if ms > MSMAX:
        raise ValueError(f"{who}: mid / share_planes = {ms} exceeds {MSMAX}")
    if B < 1 or B > MAX_B:
        raise ValueError(f"{who}: B {B} outside [1, {MAX_B}]")
    if B * N * max(2 * rel + mid, k * ms) >= _LIM or N * k >= _LIM:
        raise ValueError(f"{who}: B * N * max(2 rel + mid, k ms) and N * k must stay below 2^31")
    return ms


class SaFn(Function):
    """(P [B*N, 2 rel + mid], idx int32 [B,N,k], Wa [ms, rel (k+1)], Wb [k ms, ms], bb [k ms], rel, mid,
    share_planes) -> o [B*N, mid]. record: optional dict that receives o, h and w."""

    @staticmethod
    def forward(ctx, P, idx, Wa, Wb, bb, rel, mid, share_planes, record=None):
        who = "SaFn"
        _i32(who, "idx", idx, (None, None, None))
        B, N, k = idx.shape
        rel, mid, share_planes = int(rel), int(mid), int(share_planes)
        ms = sa_check(who, B, N, k, rel, mid, share_planes)
        _f32(who, "P", P, (B * N, 2 * rel + mid))
        _f32(who, "Wa", Wa, (ms, rel * (k + 1)))
        _f32(who, "Wb", Wb, (k * ms, ms))
        _f32(who, "bb", bb, (k * ms,))
        _lib.require_device(P, idx, Wa, Wb, bb)
        P, idx, Wa, Wb, bb = P.contiguous(), idx.contiguous(), Wa.contiguous(), Wb.contiguous(), bb.contiguous()
        dev = P.device
        o = torch.empty(B * N, mid, device=dev)
        h = torch.empty(B * N, ms, device=dev)
        w = torch.empty(B * N, k * ms, device=dev)
        _lib.call("ured_vrc_sa_fwd", _p(P), _p(idx), _p(Wa), _p(Wb), _p(bb), B, N, k, rel, mid, ms, _p(o), _p(h), _p(w),
                  _lib.stream_of(P))
        if record is not None:
            record.update(o=o, h=h, w=w)
        ctx.save_for_backward(P, idx, Wa, Wb, o, h, w)
        ctx.dims = (B, N, k, rel, mid, ms)
        return o

    @staticmethod
    def backward(ctx, go):
        P, idx, Wa, Wb, o, h, w = ctx.saved_tensors
        B, N, k, rel, mid, ms = ctx.dims
        BN, L, T = B * N, rel * (k + 1), k * ms
        dev = P.device
        go = go.contiguous()
        chunk = max(WA_MIN_CHUNK, (BN + WA_CHUNKS - 1) // WA_CHUNKS)
        nch = (BN + chunk - 1) // chunk
        gm = torch.empty(BN, mid, device=dev)
        dw = torch.empty(BN, T, device=dev)
        dh = torch.empty(BN, ms, device=dev)
        dP = torch.empty_like(P)
        ws = torch.empty(nch, ms * L, device=dev)
        _lib.call("ured_vrc_sa_bwd", _p(go), _p(o), _p(P), _p(idx), _p(Wa), _p(Wb), _p(h), _p(w), B, N, k, rel, mid, ms,
                  chunk, _p(gm), _p(dw), _p(dh), _p(dP), _p(ws), _lib.stream_of(P))
        dWa = K.colsum(ws).view(ms, L)
        dWb = torch.empty(T, ms, device=dev)
        K.wgrad(dw, T, h, ms, T, ms, BN, dWb, ms)
        dbb = K.colsum(dw)
        return dP, None, dWa, dWb, dbb, None, None, None, None


def _branches(who, ys, B):
    if not 1 <= len(ys) <= MMAX:
        raise ValueError(f"{who}: {len(ys)} branches, expected 1..{MMAX}")
    _f32(who, "y_0", ys[0], (None, None))
    R, C = ys[0].shape
    B = int(B)
    if B < 1 or B > MAX_B or R % B or R < 1 or C < 1:
        raise ValueError(f"{who}: {R} rows do not split into B = {B} clouds (1 <= B <= {MAX_B})")
    for i, y in enumerate(ys):
        _f32(who, f"y_{i}", y, (R, C))
    if R * C >= _LIM:
        raise ValueError(f"{who}: B * N * C must stay below 2^31")
    return B, R // B, C


def _four(ts):
    return [_p(t) for t in ts] + [None] * (MMAX - len(ts))


class SkMeanFn(Function):
    """(B, y_0 .. y_{m-1} [B*N, C]) -> s [B, C] = mean over the cloud's points of sum_i relu(y_i)."""

    @staticmethod
    def forward(ctx, B, *ys):
        who = "SkMeanFn"
        B, N, C = _branches(who, ys, B)
        _lib.require_device(*ys)
        ys = [y.contiguous() for y in ys]
        s = torch.empty(B, C, device=ys[0].device)
        _lib.call("ured_vrc_sk_mean_fwd", *_four(ys), len(ys), B, N, C, _p(s), _lib.stream_of(s))
        ctx.save_for_backward(*ys)
        ctx.dims = (B, N, C)
        return s

    @staticmethod
    def backward(ctx, ds):
        ys = ctx.saved_tensors
        B, N, C = ctx.dims
        ds = ds.contiguous()
        out = []
        for i, y in enumerate(ys):
            if not ctx.needs_input_grad[1 + i]:
                out.append(None)
                continue
            dy = torch.empty_like(y)
            _lib.call("ured_vrc_sk_mean_bwd", _p(y), _p(ds), B, N, C, _p(dy), _lib.stream_of(y))
            out.append(dy)
        return (None, *out)


class SkMixFn(Function):
    """(a [B, m, C], relu, y_0 .. y_{m-1} [B*N, C]) -> relu?(sum_i a[b][i][c] relu(y_i)) [B*N, C]."""

    @staticmethod
    def forward(ctx, a, relu_out, *ys):
        who = "SkMixFn"
        _f32(who, "a", a, (None, None, None))
        B, N, C = _branches(who, ys, a.shape[0])
        _f32(who, "a", a, (B, len(ys), C))
        _lib.require_device(a, *ys)
        a = a.contiguous()
        ys = [y.contiguous() for y in ys]
        out = torch.empty(B * N, C, device=a.device)
        _lib.call("ured_vrc_sk_mix_fwd", *_four(ys), _p(a), len(ys), B, N, C, int(bool(relu_out)), _p(out),
                  _lib.stream_of(out))
        ctx.save_for_backward(a, out, *ys)
        ctx.dims = (B, N, C, bool(relu_out))
        return out

    @staticmethod
    def backward(ctx, g):
        a, out, *ys = ctx.saved_tensors
        B, N, C, relu_out = ctx.dims
        g = g.contiguous()
        dys = [torch.empty_like(y) for y in ys]
        da = torch.empty_like(a)
        _lib.call("ured_vrc_sk_mix_bwd", _p(g), _p(out), *_four(ys), _p(a), len(ys), B, N, C, int(relu_out), *_four(dys),
                  _p(da), _lib.stream_of(g))
        return (da, None, *dys)


class EdgePoolFn(Function):
    """(feat [B,N,C], p_idx int32 [B,S], pn_idx int32 [B,S,pk]) -> (out [B*S, 2C], slot uint8 [B,S,C]):
    columns 0..C-1 the centre row feat[p_idx[s]], columns C..2C-1 max_j feat[pn_idx[s,j]] with the
    lowest j on a tie, slot the winning j. The backward routes to the centre row and to the winning
    neighbour only."""

    @staticmethod
    def forward(ctx, feat, p_idx, pn_idx):
        who = "EdgePoolFn"
        _f32(who, "feat", feat, (None, None, None))
        B, N, C = feat.shape
        _i32(who, "p_idx", p_idx, (B, None))
        S = p_idx.shape[1]
        _i32(who, "pn_idx", pn_idx, (B, S, None))
        pk = pn_idx.shape[2]
        if not 1 <= pk <= PKMAX:
            raise ValueError(f"{who}: pk {pk} outside [1, {PKMAX}]")
        if B < 1 or B > MAX_B or N < 1 or S < 1 or C < 1:
            raise ValueError(f"{who}: bad sizes B={B} N={N} S={S} C={C}")
        if B * N * C >= _LIM or 2 * B * S * C >= _LIM or B * S * pk >= _LIM:
            raise ValueError(f"{who}: B * N * C, 2 * B * S * C and B * S * pk must stay below 2^31")
        _lib.require_device(feat, p_idx, pn_idx)
        feat, p_idx, pn_idx = feat.contiguous(), p_idx.contiguous(), pn_idx.contiguous()
        out = torch.empty(B * S, 2 * C, device=feat.device)
        slot = torch.empty(B, S, C, dtype=torch.uint8, device=feat.device)
        _lib.call("ured_vrc_pool_fwd", _p(feat), _p(p_idx), _p(pn_idx), B, N, S, pk, C, _p(out), _p(slot),
                  _lib.stream_of(feat))
        ctx.save_for_backward(p_idx, pn_idx, slot)
        ctx.dims = (B, N, S, pk, C)
        ctx.mark_non_differentiable(slot)
        return out, slot

    @staticmethod
    def backward(ctx, g, _gs):
        p_idx, pn_idx, slot = ctx.saved_tensors
        B, N, S, pk, C = ctx.dims
        g = g.contiguous()
        dfeat = torch.empty(B, N, C, device=g.device)
        _lib.call("ured_vrc_pool_bwd", _p(g), _p(p_idx), _p(pn_idx), _p(slot), B, N, S, pk, C, _p(dfeat), _lib.stream_of(g))
        return dfeat, None, None


class UnpoolFn(Function):
    """(feat2 [B,S,D2], idx int32 [B,N,K], weight [B,N,K], skip [B,N,D1] | None), K <= 3 -> [B*N, D2 + D1]:
    sum_q weight[n][q] feat2[idx[n][q]] in columns 0..D2-1, the skip features after them (the column
    order of the reference's torch.cat([x, x_skip], 1)). Gradients go to feat2 and skip only."""

    @staticmethod
    def forward(ctx, feat2, idx, weight, skip):
        who = "UnpoolFn"
        _f32(who, "feat2", feat2, (None, None, None))
        B, S, D2 = feat2.shape
        _i32(who, "idx", idx, (B, None, None))
        N, Kq = idx.shape[1], idx.shape[2]
        if not 1 <= Kq <= 3:
            raise ValueError(f"{who}: K {Kq} outside [1, 3]")
        _f32(who, "weight", weight, (B, N, Kq))
        D1 = 0
        if skip is not None:
            _f32(who, "skip", skip, (B, N, None))
            D1 = skip.shape[2]
            if D1 < 1:
                raise ValueError(f"{who}: skip has no channels")
        if B < 1 or B > MAX_B or N < 1 or S < 1 or D2 < 1:
            raise ValueError(f"{who}: bad sizes B={B} N={N} S={S} D2={D2}")
        if B * N * (D2 + D1) >= _LIM or B * S * D2 >= _LIM:
            raise ValueError(f"{who}: B * N * (D2 + D1) and B * S * D2 must stay below 2^31")
        _lib.require_device(feat2, idx, weight, skip)
        feat2, idx, weight = feat2.contiguous(), idx.contiguous(), weight.detach().contiguous()
        skip = None if skip is None else skip.contiguous()
        out = torch.empty(B * N, D2 + D1, device=feat2.device)
        _lib.call("ured_vrc_unpool_fwd", _p(feat2), _p(idx), _p(weight), _p(skip), B, N, S, Kq, D2, D1, _p(out),
                  _lib.stream_of(out))
        ctx.save_for_backward(idx, weight)
        ctx.dims = (B, N, S, Kq, D2, D1)
        return out

    @staticmethod
    def backward(ctx, g):
        idx, weight = ctx.saved_tensors
        B, N, S, Kq, D2, D1 = ctx.dims
        g = g.contiguous()
        d2 = torch.empty(B, S, D2, device=g.device)
        ds = torch.empty(B, N, D1, device=g.device) if D1 else None
        _lib.call("ured_vrc_unpool_bwd", _p(g), _p(idx), _p(weight), B, N, S, Kq, D2, D1, _p(d2), _p(ds), _lib.stream_of(g))
        return d2, None, None, ds


def ef_check(who, B, N, k, W):
    """The limits of the edge-row kernels; W is the row width (O, or O * step_ratio)."""
    if not 1 <= k <= KMAX:
        raise ValueError(f"{who}: k {k} outside [1, {KMAX}]")
    if k > N:
        raise ValueError(f"{who}: k {k} exceeds the cloud's {N} points")
    if not 1 <= W <= OMAX * RMAX:
        raise ValueError(f"{who}: width {W} outside [1, {OMAX * RMAX}]")
    if B < 1 or B > MAX_B:
        raise ValueError(f"{who}: B {B} outside [1, {MAX_B}]")
    if B * N * k * W >= _LIM or 2 * B * N * W >= _LIM:
        raise ValueError(f"{who}: B * N * k * W and 2 * B * N * W must stay below 2^31")


class EfEdgeFn(Function):
    """(P [B*N, 2 W] = [centre | neighbour], idx int32 [B, N, k], G [B*N*k, W] | None) -> [B*N*k, W]:
    relu((G[(n, j)] + P[n, :W]) + P[idx[n, j], W:]); an index outside [0, N) reads as a zero neighbour row
    and takes no gradient. The backward returns dP (centre half summed over j, neighbour half scattered in
    ascending (n, j)) and dG. record: optional dict that receives the output."""

    @staticmethod
    def forward(ctx, P, idx, G=None, record=None):
        who = "EfEdgeFn"
        _i32(who, "idx", idx, (None, None, None))
        B, N, k = idx.shape
        _f32(who, "P", P, (B * N, None))
        if P.shape[1] < 2 or P.shape[1] % 2:
            raise ValueError(f"{who}: P has {P.shape[1]} columns, expected [centre | neighbour] halves")
        W = P.shape[1] // 2
        ef_check(who, B, N, k, W)
        if G is not None:
            _f32(who, "G", G, (B * N * k, W))
        _lib.require_device(P, idx, G)
        P, idx = P.contiguous(), idx.contiguous()
        G = None if G is None else G.contiguous()
        out = torch.empty(B * N * k, W, device=P.device)
        _lib.call("ured_vrc_ef_edge_fwd", _p(G), _p(P), _p(idx), B, N, k, W, _p(out), _lib.stream_of(P))
        if record is not None:
            record["out"] = out
        ctx.save_for_backward(idx, out)
        ctx.dims = (B, N, k, W, G is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        idx, out = ctx.saved_tensors
        B, N, k, W, has_g = ctx.dims
        g = g.contiguous()
        dP = torch.empty(B * N, 2 * W, device=g.device)
        dG = torch.empty_like(out) if has_g else None
        _lib.call("ured_vrc_ef_edge_bwd", _p(g), _p(out), _p(idx), B, N, k, W, _p(dG), _p(dP), _lib.stream_of(g))
        return dP, None, dG, None


class EfMaxFn(Function):
    """(H [B*N*k*r, O] read as [n, j, s, c], B, N, k, r) -> (out [B*N*r, O] = max over j, slot uint8 [B*N*r, O],
    the lowest j on a tie); the winner alone takes the gradient."""

    @staticmethod
    def forward(ctx, H, B, N, k, r):
        who = "EfMaxFn"
        B, N, k, r = int(B), int(N), int(k), int(r)
        if B < 1 or N < 1:
            raise ValueError(f"{who}: bad sizes B={B} N={N}")
        if not 1 <= k <= KMAX:
            raise ValueError(f"{who}: k {k} outside [1, {KMAX}]")
        if not 1 <= r <= RMAX:
            raise ValueError(f"{who}: step ratio {r} outside [1, {RMAX}]")
        _f32(who, "H", H, (B * N * k * r, None))
        O = H.shape[1]
        if not 1 <= O <= OMAX:
            raise ValueError(f"{who}: O {O} outside [1, {OMAX}]")
        if B * N * k * r * O >= _LIM:
            raise ValueError(f"{who}: B * N * k * r * O must stay below 2^31")
        _lib.require_device(H)
        H = H.contiguous()
        out = torch.empty(B * N * r, O, device=H.device)
        slot = torch.empty(B * N * r, O, dtype=torch.uint8, device=H.device)
        _lib.call("ured_vrc_ef_max_fwd", _p(H), B, N, k, r, O, _p(out), _p(slot), _lib.stream_of(H))
        ctx.save_for_backward(slot)
        ctx.dims = (B, N, k, r, O)
        ctx.mark_non_differentiable(slot)
        return out, slot

    @staticmethod
    def backward(ctx, g, _gs):
        slot, = ctx.saved_tensors
        B, N, k, r, O = ctx.dims
        g = g.contiguous()
        dH = torch.empty(B * N * k * r, O, device=g.device)
        _lib.call("ured_vrc_ef_max_bwd", _p(g), _p(slot), B, N, k, r, O, _p(dH), _lib.stream_of(g))
        return dH, None, None, None, None


class FoldFn(Function):
    """(U [R, Co], T [r, Co]) -> relu(U[n] + T[s]) [R * r, Co], row n r + s. dU sums over s ascending; dT from
    per-chunk partials (points ascending inside a chunk), then the column sums over the chunks."""

    @staticmethod
    def forward(ctx, U, T):
        who = "FoldFn"
        _f32(who, "U", U, (None, None))
        R, Co = U.shape
        _f32(who, "T", T, (None, Co))
        r = T.shape[0]
        if not 1 <= r <= RMAX:
            raise ValueError(f"{who}: step ratio {r} outside [1, {RMAX}]")
        if R < 1 or Co < 1 or R * r * Co >= _LIM:
            raise ValueError(f"{who}: bad sizes R={R} Co={Co} (R * r * Co must stay below 2^31)")
        _lib.require_device(U, T)
        U, T = U.contiguous(), T.contiguous()
        out = torch.empty(R * r, Co, device=U.device)
        _lib.call("ured_vrc_fold_fwd", _p(U), _p(T), 1, R, r, Co, _p(out), _lib.stream_of(U))
        ctx.save_for_backward(out)
        ctx.dims = (R, r, Co)
        return out

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        R, r, Co = ctx.dims
        g = g.contiguous()
        chunk = max(FOLD_MIN_CHUNK, (R + FOLD_CHUNKS - 1) // FOLD_CHUNKS)
        nch = (R + chunk - 1) // chunk
        dU = torch.empty(R, Co, device=g.device)
        ws = torch.empty(nch, r * Co, device=g.device)
        _lib.call("ured_vrc_fold_bwd", _p(g), _p(out), 1, R, r, Co, chunk, _p(dU), _p(ws), _lib.stream_of(g))
        return dU, K.colsum(ws).view(r, Co)


def latent_check(who, B, Z):
    """The limits of the latent-head kernels."""
    if not 1 <= Z <= ZMAX:
        raise ValueError(f"{who}: Z {Z} outside [1, {ZMAX}]")
    if B < 1 or B > MAX_B:
        raise ValueError(f"{who}: B {B} outside [1, {MAX_B}]")
    if 2 * B * Z >= _LIM:
        raise ValueError(f"{who}: 2 * B * Z must stay below 2^31")


class LatentFn(Function):
    """(oq [B, 2Z], op [B, 2Z], eps_q [B, Z], eps_p [B, Z]) -> (z [2B, Z], kl_rec [B, Z], kl_g [B, Z]); with
    op = eps_p = None (evaluation) -> z [B, Z], and kl_rec / kl_g are None. mu = o[:, :Z], s = softplus(o[:, Z:]);
    z = [mu_q + s_q eps_q; mu_p + s_p eps_p], kl_rec = KL(N(0,1) || N(mu_p, s_p)), kl_g = KL(N(mu_p, s_p) ||
    N(mu_q, s_q)) with the prior detached. eps takes no gradient."""

    @staticmethod
    def forward(ctx, oq, op, eps_q, eps_p):
        who = "LatentFn"
        _f32(who, "oq", oq, (None, None))
        B, W = oq.shape
        if W < 2 or W % 2:
            raise ValueError(f"{who}: oq has {W} columns, expected [mu | scale] halves")
        Z = W // 2
        latent_check(who, B, Z)
        _f32(who, "eps_q", eps_q, (B, Z))
        if (op is None) != (eps_p is None):
            raise ValueError(f"{who}: op and eps_p go together (both for training, neither for evaluation)")
        train = op is not None
        if train:
            _f32(who, "op", op, (B, 2 * Z))
            _f32(who, "eps_p", eps_p, (B, Z))
        _lib.require_device(oq, op, eps_q, eps_p)
        oq, eps_q = oq.contiguous(), eps_q.contiguous()
        dev = oq.device
        kl_rec = kl_g = None
        if train:
            op, eps_p = op.contiguous(), eps_p.contiguous()
            kl_rec, kl_g = torch.empty(B, Z, device=dev), torch.empty(B, Z, device=dev)
        z = torch.empty(2 * B if train else B, Z, device=dev)
        _lib.call("ured_vrc_latent_fwd", _p(oq), _p(op), _p(eps_q), _p(eps_p), B, Z, _p(z), _p(kl_rec), _p(kl_g),
                  _lib.stream_of(oq))
        ctx.set_materialize_grads(False)
        if train:
            ctx.save_for_backward(oq, op, eps_q, eps_p)
        else:
            ctx.save_for_backward(oq, eps_q)
        ctx.dims = (B, Z, train)
        return z, kl_rec, kl_g

    @staticmethod
    def backward(ctx, dz, dkr, dkg):
        B, Z, train = ctx.dims
        if train:
            oq, op, eps_q, eps_p = ctx.saved_tensors
        else:
            (oq, eps_q), op, eps_p = ctx.saved_tensors, None, None
            dkr = dkg = None
        dz, dkr, dkg = (None if g is None else g.contiguous() for g in (dz, dkr, dkg))
        d_oq = torch.empty_like(oq)
        d_op = torch.empty_like(op) if train else None
        _lib.call("ured_vrc_latent_bwd", _p(oq), _p(op), _p(eps_q), _p(eps_p), _p(dz), _p(dkr), _p(dkg), B, Z, _p(d_oq),
                  _p(d_op), _lib.stream_of(oq))
        return d_oq, d_op, None, None


def gauss_check(who, n, m, Z):
    """The limits of the Gaussian-kernel kernels."""
    if not 1 <= n <= GAUSS_MAX or not 1 <= m <= GAUSS_MAX:
        raise ValueError(f"{who}: n {n} or m {m} outside [1, {GAUSS_MAX}]")
    if not 1 <= Z <= ZMAX:
        raise ValueError(f"{who}: Z {Z} outside [1, {ZMAX}]")


class GaussKernelFn(Function):
    """(x [n, Z], y [m, Z]) -> K [n, m] = exp(-mean_d((x_i - y_j)^2) / Z) from direct differences (equal rows give
    exactly 1); dx sums over j ascending, dy over i ascending. x and y may be the same tensor: autograd adds
    the two roles' gradients."""

    @staticmethod
    def forward(ctx, x, y):
        who = "GaussKernelFn"
        _f32(who, "x", x, (None, None))
        n, Z = x.shape
        _f32(who, "y", y, (None, Z))
        m = y.shape[0]
        gauss_check(who, n, m, Z)
        _lib.require_device(x, y)
        x, y = x.contiguous(), y.contiguous()
        K_ = torch.empty(n, m, device=x.device)
        _lib.call("ured_vrc_gauss_fwd", _p(x), _p(y), n, m, Z, _p(K_), _lib.stream_of(x))
        ctx.save_for_backward(x, y, K_)
        ctx.set_materialize_grads(False)
        return K_

    @staticmethod
    def backward(ctx, dK):
        if dK is None:
            return None, None
        x, y, K_ = ctx.saved_tensors
        dx, dy = torch.empty_like(x), torch.empty_like(y)
        _lib.call("ured_vrc_gauss_bwd", _p(x), _p(y), _p(K_), _p(dK.contiguous()), x.shape[0], y.shape[0], x.shape[1], _p(dx),
                  _p(dy), _lib.stream_of(x))
        return dx, dy


class CenterFn(Function):
    """(y [R*r, 3], cp [R, 3]) -> y[n r + s] + cp[n] (ured_pcn_center_fwd); dcp sums over s ascending."""

    @staticmethod
    def forward(ctx, y, cp):
        who = "CenterFn"
        _f32(who, "cp", cp, (None, 3))
        R = cp.shape[0]
        _f32(who, "y", y, (None, 3))
        if R < 1 or y.shape[0] < R or y.shape[0] % R or y.shape[0] // R > RMAX:
            raise ValueError(f"{who}: {y.shape[0]} rows are not 1..{RMAX} copies of {R} centres")
        _lib.require_device(y, cp)
        ctx.dims = (R, y.shape[0] // R)
        return center_fwd(y.contiguous(), cp.contiguous(), 1, R, y.shape[0] // R)

    @staticmethod
    def backward(ctx, g):
        R, r = ctx.dims
        g = g.contiguous()
        return g, center_bwd(g, None, 1, R, r)


class ReluFn(Function):
    """max(x, 0) by ured_pcn_relu; the backward passes g where the output is positive."""

    @staticmethod
    def forward(ctx, x):
        _lib.require_device(x)
        out = relu(x.contiguous())
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        out, = ctx.saved_tensors
        return relu(out, g.contiguous())


class LinearRowsFn(Function):
    """y [M, Co] = act(x [M, Ci]) @ W [Co, Ci]^T (+ b) (+ rowbias[row // group_rows]); act = ReLU when
    relu_in (the GEMM's A prologue), else the identity. x may be a column slice of a wider row-major
    matrix (its row stride is the GEMM's lda)."""

    @staticmethod
    def forward(ctx, x, W, b, relu_in, rowbias, group_rows):
        who = "LinearRowsFn"
        _f32(who, "x", x, (None, None))
        M, Ci = x.shape
        _f32(who, "W", W, (None, Ci))
        Co = W.shape[0]
        if b is not None:
            _f32(who, "b", b, (Co,))
        if rowbias is not None:
            _f32(who, "rowbias", rowbias, (None, Co))
            if group_rows < 1 or rowbias.shape[0] * group_rows != M:
                raise ValueError(f"{who}: rowbias {tuple(rowbias.shape)} x group_rows {group_rows} does not cover {M} rows")
        if M < 1 or M * max(Ci, Co) >= _LIM:
            raise ValueError(f"{who}: M {M} must be at least 1 and M * channels below 2^31")
        _lib.require_device(x, W, b, rowbias)
        if x.stride(1) != 1 or x.stride(0) < Ci:
            x = x.contiguous()
        W = W.contiguous()
        b = None if b is None else b.contiguous()
        dev = x.device
        rl = _Relu(Ci, dev) if relu_in else None
        y = torch.empty(M, Co, device=dev)
        kw = {} if rl is None else rl.kw(Ci)
        if rowbias is not None:
            rowbias = rowbias.contiguous()
            sws = torch.empty(K.nblocks(M), 2, Co, device=dev)      # the epilogue's statistics partials: unused
            K.gemm(M, Co, Ci, x, x.stride(0), W, Ci, y, Co, bias=b, epi=K.EPI_FWD, stat_ws=sws, rowbias=rowbias, ldr=Co,
                   group_rows=int(group_rows), **kw)
        else:
            K.gemm(M, Co, Ci, x, x.stride(0), W, Ci, y, Co, bias=b, **kw)
        ctx.save_for_backward(x, W)
        ctx.cfg = (bool(relu_in), b is not None, rowbias is not None, int(group_rows) if rowbias is not None else 0)
        return y

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        relu_in, has_b, has_rb, group_rows = ctx.cfg
        need = ctx.needs_input_grad
        M, Ci = x.shape
        Co = W.shape[0]
        dev = g.device
        g = g.contiguous()
        dx = dW = db = drb = None
        if need[0]:
            dx = torch.empty(M, Ci, device=dev)
            K.gemm(M, Ci, Co, g, Co, W, Ci, dx, Ci, b_kmajor=True)
            if relu_in:
                dx = relu(x.contiguous(), dx)
        if need[1]:
            dW = torch.empty(Co, Ci, device=dev)
            kw = {}
            if relu_in:
                rl = _Relu(Ci, dev)
                kw = {"pro": K.PRO_ENC, "pro_s": rl.s, "pro_t": rl.t}
            K.wgrad(g, Co, x, x.stride(0), Co, Ci, M, dW, Ci, **kw)
        if has_b and need[2]:
            db = K.colsum(g)
        if has_rb and need[4]:
            drb = K.group_colsum(g, Co, M // group_rows, group_rows=group_rows)
        return dx, dW, db, None, drb, None


def linear_rows(x, W, b=None, relu_in=False, rowbias=None, group_rows=0):
    return LinearRowsFn.apply(x, W, b, relu_in, rowbias, group_rows)


class MaxRowsFn(Function):
    """x [B*N, C] -> (max over each cloud's N rows [B, C], the winning row of the [B*N] matrix int32
    [B, C], the lowest on a tie); the winner alone takes the gradient."""

    @staticmethod
    def forward(ctx, x, N):
        _f32("MaxRowsFn", "x", x, (None, None))
        if N < 1 or x.shape[0] % N:
            raise ValueError(f"MaxRowsFn: {x.shape[0]} rows do not split into clouds of {N}")
        _lib.require_device(x)
        x = x.contiguous()
        C = x.shape[1]
        rl = _Relu(C, x.device)
        out, win = K.pool_rows(x, int(N), rl.s, rl.t, relu=False)
        ctx.save_for_backward(win)
        ctx.N = int(N)
        ctx.mark_non_differentiable(win)
        return out, win

    @staticmethod
    def backward(ctx, g, _gw):
        win, = ctx.saved_tensors
        return pool_bwd(g.contiguous(), win, ctx.N), None
