"""The PCN completion network (Density_aware_Chamfer_Distance/models/pcn.py:13-71) as two autograd
Functions on libured_hip.so: every matrix product is ured_gemm (ured_hip.kernels), the rest the
kernels of csrc/pcn.hip. Activations are point-major [rows][C] fp32.

PcnEncoderFn: conv1 -> ReLU -> conv2 -> max over points -> conv3 on [point feature | global feature]
  -> ReLU -> conv4 -> max over points. The cat with the repeated global feature is never built:
  conv3 is a GEMM over the 256 point channels plus a per-cloud row bias global @ W3[:, 256:]^T
  (the rowbias / group_rows epilogue). Both max-pools keep the winning point per (cloud, channel),
  lowest index on a tie; the winner alone takes the gradient.
PcnDecoderFn: fc1 -> ReLU -> fc2 -> ReLU -> fc3 -> coarse; conv1 on [grid | coarse point | global
  feature] -> ReLU -> conv2 -> ReLU -> conv3 -> + coarse point -> fine. The [B, 1029, num_fine]
  operand is never built: conv1's pre-activation of fine point (b, c, s) is Gb[b] + Pc[b, c] + Gs[s],
  three small GEMMs and ured_pcn_fold_fwd; ured_pcn_fold_bwd reduces the gradient back.
A ReLU between two GEMMs is the second one's A prologue (max(x * 1 + 0, 0)); only pre-activations
are kept. Caller's stream, no host synchronisation.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _lib
from . import kernels as K

_P, _I, _LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_lib.register({
    "ured_pcn_relu": [_P, _P, _LL, _P, _P],
    "ured_pcn_pool_bwd": [_P, _P, _I, _I, _I, _P, _I, _P],
    "ured_pcn_fold_fwd": [_P, _P, _P, _I, _I, _I, _I, _P, _P],
    "ured_pcn_fold_bwd": [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "ured_pcn_center_fwd": [_P, _P, _I, _I, _I, _P, _P],
    "ured_pcn_center_bwd": [_P, _P, _I, _I, _I, _P, _P],
})

MAX_SCALE = 16          # PCN_MAX_SCALE (csrc/pcn.hip)
FOLD_CHUNK = 32         # coarse points per workgroup of ured_pcn_fold_bwd
_LIM = 1 << 31


def _p(t):
    return None if t is None else t.data_ptr()


def _f32(who, name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be a float32 tensor")
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {shape}")


def relu(y, g=None):
    """max(y, 0), or with g the ReLU backward: g where y > 0, else 0."""
    out = torch.empty_like(y)
    _lib.call("ured_pcn_relu", _p(y), _p(g), y.numel(), _p(out), _lib.stream_of(y))
    return out


def pool_bwd(g, win, rows, dY=None):
    """Backward of the max over each group's `rows` rows: a new dY [G*rows, C] written everywhere, or
    g added at the winners of a given dY."""
    G, C = g.shape
    new = dY is None
    if new:
        dY = torch.empty(G * rows, C, device=g.device)
    _lib.call("ured_pcn_pool_bwd", _p(g), _p(win), G, rows, C, _p(dY), int(not new), _lib.stream_of(g))
    return dY


def fold_fwd(Gb, Pc, Gs, B, nc, S):
    C = Gb.shape[1]
    Y = torch.empty(B * nc * S, C, device=Gb.device)
    _lib.call("ured_pcn_fold_fwd", _p(Gb), _p(Pc), _p(Gs), B, nc, S, C, _p(Y), _lib.stream_of(Y))
    return Y


def fold_bwd(dH, Y, B, nc, S):
    """-> (dGb [B,C], dPc [B*nc,C], dGs [S,C]) of G = dH where Y > 0 else 0."""
    C = Y.shape[1]
    nchunks = (B * nc + FOLD_CHUNK - 1) // FOLD_CHUNK
    dPc = torch.empty(B * nc, C, device=Y.device)
    ws = torch.empty(nchunks, S * C, device=Y.device)
    _lib.call("ured_pcn_fold_bwd", _p(dH), _p(Y), B, nc, S, C, FOLD_CHUNK, _p(dPc), _p(ws), _lib.stream_of(Y))
    dGs = K.colsum(ws).view(S, C)
    dGb = K.group_colsum(dPc, C, B, group_rows=nc)
    return dGb, dPc, dGs


def center_fwd(y, cp, B, nc, S):
    out = torch.empty_like(y)
    _lib.call("ured_pcn_center_fwd", _p(y), _p(cp), B, nc, S, _p(out), _lib.stream_of(y))
    return out


def center_bwd(dF, add, B, nc, S):
    out = torch.empty(B * nc, 3, device=dF.device)
    _lib.call("ured_pcn_center_bwd", _p(dF), _p(add), B, nc, S, _p(out), _lib.stream_of(dF))
    return out


class _Relu:
    """scale 1 / shift 0 vectors of the GEMM's ReLU prologue, max(x * 1 + 0, 0)."""

    def __init__(self, n, dev, s=None, t=None):
        self.s = torch.ones(n, device=dev) if s is None else s
        self.t = torch.zeros(n, device=dev) if t is None else t

    def kw(self, k, name="pro_a"):
        return {name: K.PRO_ENC, "pro_s": self.s[:k], "pro_t": self.t[:k]}


def _lin(x, W, b, rl=None):
    """[M,K] @ W [N,K]^T + b; rl: the ReLU of x as the A prologue."""
    M, Kd = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, device=x.device)
    K.gemm(M, N, Kd, x, Kd, W, Kd, y, N, bias=b, **({} if rl is None else rl.kw(Kd)))
    return y


def _dgrad(g, W):
    """g [M,N] @ W [N,K] -> [M,K]."""
    M, N = g.shape
    Kd = W.shape[1]
    dx = torch.empty(M, Kd, device=g.device)
    K.gemm(M, Kd, N, g, N, W, Kd, dx, Kd, b_kmajor=True)
    return dx


def _wgrad(g, x, rl=None):
    """g [M,N]^T @ act(x) [M,K] -> [N,K]; rl: the ReLU of x as the prologue."""
    M, N = g.shape
    Kd = x.shape[1]
    dW = torch.empty(N, Kd, device=g.device)
    kw = {} if rl is None else {"pro": K.PRO_ENC, "pro_s": rl.s[:Kd], "pro_t": rl.t[:Kd]}
    K.wgrad(g, N, x, Kd, N, Kd, M, dW, Kd, **kw)
    return dW


def _w2(w):
    return w.reshape(w.shape[0], -1).contiguous()


class PcnEncoderFn(Function):
    """(x [B,3,N], conv1..conv4 weight [Co,Ci,1] and bias) -> global feature [B, Co4].
    record: optional dict; the forward stores the pre-activations Y1..Y4 ([B*N, C]) and the winners
    win1 / win2 (int32 [B, C], rows of the [B*N] matrix) there."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, w4, b4, record=None):
        who = "PcnEncoderFn"
        _f32(who, "x", x, (None, 3, None))
        _lib.require_device(x, w1, b1, w2, b2, w3, b3, w4, b4)
        B, _, N = x.shape
        if B < 1 or N < 1:
            raise ValueError(f"{who}: empty input {tuple(x.shape)}")
        W1, W2, W3, W4 = _w2(w1), _w2(w2), _w2(w3), _w2(w4)
        C1, C2, C3, C4 = W1.shape[0], W2.shape[0], W3.shape[0], W4.shape[0]
        _f32(who, "conv1.weight", W1, (C1, 3))
        _f32(who, "conv2.weight", W2, (C2, C1))
        _f32(who, "conv3.weight", W3, (C3, 2 * C2))
        _f32(who, "conv4.weight", W4, (C4, C3))
        for name, b, c in (("conv1", b1, C1), ("conv2", b2, C2), ("conv3", b3, C3), ("conv4", b4, C4)):
            _f32(who, name + ".bias", b, (c,))
        M = B * N
        if M * max(C1, C2, C3, C4) >= _LIM or B > 65535:
            raise ValueError(f"{who}: B * N * channels must stay below 2^31 and B below 65536")
        dev = x.device
        rl = _Relu(max(C1, C2, C3, C4), dev)
        X = x.transpose(1, 2).contiguous().view(M, 3)
        Y1 = _lin(X, W1, b1.contiguous())
        Y2 = _lin(Y1, W2, b2.contiguous(), rl)
        g1, win1 = K.pool_rows(Y2, N, rl.s[:C2], rl.t[:C2], relu=False)
        W3a, W3b = W3[:, :C2].contiguous(), W3[:, C2:].contiguous()
        R3 = _lin(g1, W3b, None)                       # per-cloud row bias of conv3
        Y3 = torch.empty(M, C3, device=dev)
        sws = torch.empty(K.nblocks(M), 2, C3, device=dev)     # the epilogue's statistics partials: unused
        K.gemm(M, C3, C2, Y2, C2, W3a, C2, Y3, C3, bias=b3.contiguous(), epi=K.EPI_FWD, stat_ws=sws,
               rowbias=R3, ldr=C3, group_rows=N)
        Y4 = _lin(Y3, W4, b4.contiguous(), rl)
        feat, win2 = K.pool_rows(Y4, N, rl.s[:C4], rl.t[:C4], relu=False)
        if record is not None:
            record.update(Y1=Y1, Y2=Y2, Y3=Y3, Y4=Y4, win1=win1, win2=win2)
        ctx.save_for_backward(X, Y1, Y2, Y3, g1, win1, win2, W1, W2, W3a, W3b, W4, rl.s, rl.t)
        ctx.dims = (B, N)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        X, Y1, Y2, Y3, g1, win1, win2, W1, W2, W3a, W3b, W4, rs, rt = ctx.saved_tensors
        B, N = ctx.dims
        rl = _Relu(0, None, rs, rt)
        need = ctx.needs_input_grad
        dfeat = dfeat.contiguous()
        C2 = W2.shape[0]
        dY4 = pool_bwd(dfeat, win2, N)
        dW4 = _wgrad(dY4, Y3, rl)
        db4 = K.colsum(dfeat)
        dY3 = relu(Y3, _dgrad(dY4, W4))
        del dY4
        dW3a = _wgrad(dY3, Y2)
        dR3 = K.group_colsum(dY3, dY3.shape[1], B, group_rows=N)
        db3 = K.colsum(dR3)
        dW3b = _wgrad(dR3, g1)
        dg1 = _dgrad(dR3, W3b)
        dY2 = pool_bwd(dg1, win1, N, _dgrad(dY3, W3a))
        del dY3
        dW2 = _wgrad(dY2, Y1, rl)
        db2 = K.colsum(dY2)
        dY1 = relu(Y1, _dgrad(dY2, W2))
        dW1 = _wgrad(dY1, X)
        db1 = K.colsum(dY1)
        dx = _dgrad(dY1, W1).view(B, N, 3).transpose(1, 2) if need[0] else None
        dW3 = torch.cat((dW3a, dW3b), 1)
        return (dx, dW1.unsqueeze(-1), db1, dW2.unsqueeze(-1), db2, dW3.unsqueeze(-1), db3, dW4.unsqueeze(-1), db4, None)


class PcnDecoderFn(Function):
    """(feature [B,F], fc1..fc3 and conv1..conv3 weights and biases, grid [2,scale]) ->
    (coarse [B,3,num_coarse], fine [B,3,num_coarse*scale]); fine is the transpose of a contiguous
    point-major [B, num_fine, 3]. record: optional dict for the pre-activations A1, A2 (fc), Y1, Y2
    (conv1, conv2: [B*num_fine, C])."""

    @staticmethod
    def forward(ctx, feat, fw1, fb1, fw2, fb2, fw3, fb3, cw1, cb1, cw2, cb2, cw3, cb3, grid, record=None):
        who = "PcnDecoderFn"
        _f32(who, "feature", feat, (None, None))
        _f32(who, "grid", grid, (2, None))
        _lib.require_device(feat, fw1, fb1, fw2, fb2, fw3, fb3, cw1, cb1, cw2, cb2, cw3, cb3, grid)
        B, F = feat.shape
        S = grid.shape[1]
        W1c, W2c, W3c = _w2(cw1), _w2(cw2), _w2(cw3)
        C = W1c.shape[0]
        _f32(who, "fc1.weight", fw1, (None, F))
        _f32(who, "fc2.weight", fw2, (None, fw1.shape[0]))
        _f32(who, "fc3.weight", fw3, (None, fw2.shape[0]))
        _f32(who, "conv1.weight", W1c, (C, 5 + F))
        _f32(who, "conv2.weight", W2c, (None, C))
        _f32(who, "conv3.weight", W3c, (3, W2c.shape[0]))
        if fw3.shape[0] % 3 or B < 1:
            raise ValueError(f"{who}: fc3 must have 3 * num_coarse outputs and the batch at least one cloud")
        if not 1 <= S <= MAX_SCALE:
            raise ValueError(f"{who}: scale {S} outside [1, {MAX_SCALE}]")
        nc = fw3.shape[0] // 3
        R = B * nc * S
        if R * max(C, W2c.shape[0]) >= _LIM or B > 65535:
            raise ValueError(f"{who}: B * num_fine * channels must stay below 2^31 and B below 65536")
        dev = feat.device
        feat = feat.contiguous()
        fw1, fw2, fw3 = fw1.contiguous(), fw2.contiguous(), fw3.contiguous()
        rl = _Relu(max(C, W2c.shape[0]), dev)
        A1 = _lin(feat, fw1, fb1.contiguous())
        H1 = relu(A1)
        A2 = _lin(H1, fw2, fb2.contiguous())
        H2 = relu(A2)
        coarse = _lin(H2, fw3, fb3.contiguous()).view(B, 3, nc)
        CP = coarse.transpose(1, 2).contiguous().view(B * nc, 3)        # coarse points as rows
        Ws, Wp, Wg = W1c[:, 0:2].contiguous(), W1c[:, 2:5].contiguous(), W1c[:, 5:].contiguous()
        GT = grid.t().contiguous()                                       # [S, 2]
        Gb = _lin(feat, Wg, cb1.contiguous())
        Pc = _lin(CP, Wp, None)
        Gs = _lin(GT, Ws, None)
        Y1 = fold_fwd(Gb, Pc, Gs, B, nc, S)
        del Gb, Pc, Gs
        Y2 = _lin(Y1, W2c, cb2.contiguous(), rl)
        fine = center_fwd(_lin(Y2, W3c, cb3.contiguous(), rl), CP, B, nc, S)
        if record is not None:
            record.update(A1=A1, A2=A2, Y1=Y1, Y2=Y2)
        ctx.save_for_backward(feat, A1, H1, A2, H2, CP, GT, Y1, Y2, fw1, fw2, fw3, Ws, Wp, Wg, W2c, W3c, rl.s, rl.t)
        ctx.dims = (B, nc, S)
        ctx.set_materialize_grads(False)
        return coarse, fine.view(B, nc * S, 3).transpose(1, 2)

    @staticmethod
    def backward(ctx, dcoarse, dfine):
        feat, A1, H1, A2, H2, CP, GT, Y1, Y2, fw1, fw2, fw3, Ws, Wp, Wg, W2c, W3c, rs, rt = ctx.saved_tensors
        B, nc, S = ctx.dims
        rl = _Relu(0, None, rs, rt)
        dev = feat.device
        dfeat = None
        dCP = None
        gcw1 = gcb1 = gcw2 = gcb2 = gcw3 = gcb3 = None
        if dfine is not None:
            dF = dfine.transpose(1, 2).contiguous().view(B * nc * S, 3)
            gcw3 = _wgrad(dF, Y2, rl)
            gcb3 = K.colsum(dF)
            dY2 = relu(Y2, _dgrad(dF, W3c))
            gcw2 = _wgrad(dY2, Y1, rl)
            gcb2 = K.colsum(dY2)
            dGb, dPc, dGs = fold_bwd(_dgrad(dY2, W2c), Y1, B, nc, S)
            del dY2
            gcb1 = K.colsum(dGb)
            gcw1 = torch.cat((_wgrad(dGs, GT), _wgrad(dPc, CP), _wgrad(dGb, feat)), 1)
            dfeat = _dgrad(dGb, Wg)
            dCP = center_bwd(dF, _dgrad(dPc, Wp), B, nc, S)
        else:
            C = Wg.shape[0]
            gcw1 = torch.zeros(C, 5 + feat.shape[1], device=dev)
            gcb1, gcw2, gcb2 = torch.zeros(C, device=dev), torch.zeros_like(W2c), torch.zeros(W2c.shape[0], device=dev)
            gcw3, gcb3 = torch.zeros_like(W3c), torch.zeros(3, device=dev)
        if dCP is not None:
            dA3 = dCP.view(B, nc, 3).transpose(1, 2)
            dA3 = (dA3 + dcoarse if dcoarse is not None else dA3).reshape(B, 3 * nc).contiguous()
        elif dcoarse is not None:
            dA3 = dcoarse.reshape(B, 3 * nc).contiguous()
        else:
            dA3 = torch.zeros(B, 3 * nc, device=dev)
        gfw3, gfb3 = _wgrad(dA3, H2), K.colsum(dA3)
        dA2 = relu(A2, _dgrad(dA3, fw3))
        gfw2, gfb2 = _wgrad(dA2, H1), K.colsum(dA2)
        dA1 = relu(A1, _dgrad(dA2, fw2))
        gfw1, gfb1 = _wgrad(dA1, feat), K.colsum(dA1)
        d1 = _dgrad(dA1, fw1)
        dfeat = d1 if dfeat is None else dfeat + d1
        return (dfeat, gfw1, gfb1, gfw2, gfb2, gfw3, gfb3, gcw1.unsqueeze(-1), gcb1, gcw2.unsqueeze(-1), gcb2,
                gcw3.unsqueeze(-1), gcb3, None, None)
