"""Fused per-point MLP chains on libured_hip.so, as torch autograd Functions.

PointEncoderFn : TargetEncoder.forward (network/simple_encoder.py:88-107) —
                 conv 3->64->64 (mlp1), 64->64->128->1024 (mlp2), fuse_sem
                 (1024+S)->1024, per_point_out 1024->C->C, max-pool + fc —
                 every Conv1d+BatchNorm1d(train)+ReLU fused into ured_gemm
                 launches (prologue = previous BN+ReLU, epilogue = stats / pool).
ResidualNetFn  : re_residual_net.forward (network/deformation_net.py:96-107) with
                 FeedForwardNet_norm [in,256,256,32,3] (Conv->ReLU->BN), whose
                 input is cat(per-point features, per-group code): the group half
                 is folded into a per-group row bias (W_code @ code), so it is
                 never broadcast to every point.
PointChainFn   : the PointNet conv stacks (STN3d / STNkd / PointNetEncoder,
                 network/pointnet/pointnet_utils.py): L x Conv1d+BatchNorm1d(+ReLU),
                 then a max-pool over each cloud and/or the last activation.
All three run forward and backward entirely on HIP kernels; only the tiny
per-call index bookkeeping is Python. A chain is a loop over _layer_fwd /
_layer_bwd (one Conv+BN layer each way); a Function adds only its own special
layer (fuse_sem + pooling, the row-bias first layer, the K = 0 last layer) and
its head.
"""
from typing import Any, NamedTuple

import torch
from torch.autograd import Function

from . import _lib
from . import kernels as K
from . import node
from .optim import grad_buffer

BN_EPS = 1e-5


class EncoderSpec:
    """Static description of one TargetEncoder call.

    mode "src": x [G*group_rows, 3] with per-group semantics sem [G, S] (row bias)
    mode "tgt": x [M, 3] with per-point semantics sem [M, S] (extra K columns)
    bn_modules: the 7 BatchNorm1d modules (running stats updated in place when training)
    rw: optional K.RowWeights — group g of the call stands for rw.w[g] identical groups of
        the full batch (unique-row training: batch statistics and BN backward are those of
        the expanded batch; the caller expands outputs and sums duplicate gradients)
    record: optional dict; the forward stores the max-pool winners there ("pool_rows": int32
        [G, 1024], the row of the call each pooled channel came from)
    """

    def __init__(self, mode, group_rows, training, bn_modules, momentum=0.1, eps=BN_EPS, rw=None, record=None):
        assert mode in ("src", "tgt")
        self.mode, self.group_rows, self.training = mode, group_rows, training
        self.bn_modules, self.momentum, self.eps = bn_modules, momentum, eps
        self.rw = rw
        self.record = record


def _nbt(bnm):
    """The module's int64 num_batches_tracked (incremented inside the finalize launch)."""
    t = bnm.num_batches_tracked
    if t is None:
        return None
    if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous():
        raise TypeError("num_batches_tracked must be a contiguous int64 device tensor")
    return t


def _bn_state(bnm, training, rw, sws, M, N, gamma, beta, eps):
    """BN state of a layer from its GEMM's statistics partials (training: batch statistics, the
    module's running stats and num_batches_tracked updated in place) or its running stats (eval)."""
    if training:
        mom = bnm.momentum if bnm.momentum is not None else 0.0
        return K.bn_fwd_finalize(sws, M, N, gamma, beta, eps, mom, bnm.running_mean, bnm.running_var, rw=rw,
                                 num_batches_tracked=_nbt(bnm))
    return K.bn_eval_state(gamma, beta, bnm.running_mean, bnm.running_var, eps)


def _layer_fwd(i, params, h, Kdim, pro, st, bnm, training, rw, *, eps=BN_EPS, stat_relu=False, special=None):
    """Forward of Conv1d(k=1) + BatchNorm1d layer i of a chain (params W,b,gamma,beta at 4*i):
    Y = pro(h)[:, :Kdim] @ W^T + b in one GEMM, the previous layer's BN (st, applied in order
    `pro`) as its prologue and this layer's batch-statistics partials as its epilogue, then this
    layer's BN state. special(N) -> further GEMM arguments of a chain's one special layer; it runs
    after Y and the statistics workspace are allocated. Returns (Y, state)."""
    W = params[4 * i].reshape(params[4 * i].shape[0], -1)
    M, N = h.shape[0], W.shape[0]
    Y = torch.empty(M, N, device=h.device)
    sws = torch.empty(K.nblocks(M), 2, N, device=h.device)
    kw = {} if special is None else special(N)
    K.gemm(M, N, Kdim, h, h.shape[1], W, W.shape[1], Y, N, pro_a=pro,
           pro_s=None if st is None else st.scale, pro_t=None if st is None else st.shift,
           bias=params[4 * i + 1], epi=K.EPI_FWD, stat_ws=sws, stat_relu=stat_relu, **kw)
    return Y, _bn_state(bnm, training, rw, sws, M, N, params[4 * i + 2], params[4 * i + 3], eps)


def _require_training(spec, name):
    """_layer_bwd applies the batch-statistics BN backward (the mean and variance terms of
    bn_bwd_finalize / bn_bwd_apply). A chain that ran on running statistics (training=False) has
    the eval-BN gradient instead, scale and mask only, which no chain kernel computes: refuse
    rather than return the training formula. Inference runs under no_grad and never gets here
    (the check sits in backward because forward cannot tell a no_grad call: ctx.needs_input_grad
    is set either way)."""
    if not spec.training:
        raise RuntimeError(f"{name}: backward through a chain that ran with training=False (eval-mode BatchNorm) is "
                           "not supported; run eval-mode chains under torch.no_grad()")


def _layer_bwd(i, params, grads, bias, x, Ys, states, dY, Wn, act, pro, rw, *, Kdim=None, out_off=0, special=None,
               **kw):
    """Backward of layer i of a chain, from dY = the gradient at the output of the layer above
    and Wn = that layer's weight: the fused dgrad dH_i = dY @ Wn[:, :N] with the activation mask
    (act: K.ACT_*) and the BN-backward partials of layer i in its epilogue (Kdim = 0: no layer
    above, the gradient enters through the epilogue's kw alone), the BN-backward finalize and
    apply, the weight gradient against the layer's input (x, or the layer below's Y under its BN
    as prologue, order `pro`; out_off: first weight column), then special(dYi, cs, dW) for the
    weight columns a chain's special layer adds. The bias column sums are queued on `bias`, the
    four gradients go to grads[4*i..]. Returns (dY_i, W_i) for the layer below."""
    Y, st = Ys[i], states[i]
    M, N = Y.shape
    G_ = torch.empty(M, N, device=Y.device)
    bws = torch.empty(K.nblocks(M), 2, N, device=Y.device)
    K.gemm(M, N, dY.shape[1] if Kdim is None else Kdim, dY, dY.shape[1], Wn, Wn.shape[1], G_, N, b_kmajor=True,
           epi=K.EPI_BNBWD, Yp=Y, ldy=N, bn=st, bwd_res=act, bwd_ws=bws, **kw)
    gamma = params[4 * i + 2]
    dgamma, dbeta = grad_buffer(gamma), grad_buffer(params[4 * i + 3])
    coefs = K.bn_bwd_finalize(bws, M, N, gamma, st.invstd, dgamma, dbeta, rw=rw)
    dYi, cs = K.bn_bwd_apply(G_, Y, act == K.ACT_RES, st.mean, coefs, rw=rw)
    W = params[4 * i].reshape(params[4 * i].shape[0], -1)
    dW, db = grad_buffer(params[4 * i]).view(W.shape), grad_buffer(params[4 * i + 1])
    X, stp = (x, None) if i == 0 else (Ys[i - 1], states[i - 1])
    kin = X.shape[1]
    K.wgrad(dYi, N, X, kin, N, kin, M, dW, W.shape[1], out_off=out_off, pro=K.PRO_NONE if stp is None else pro,
            pro_s=None if stp is None else stp.scale, pro_t=None if stp is None else stp.shift)
    if special is not None:
        special(dYi, cs, dW)
    bias.add(cs, db)
    grads[4 * i] = dW.view(params[4 * i].shape)
    grads[4 * i + 1] = db
    grads[4 * i + 2], grads[4 * i + 3] = dgamma, dbeta
    return dYi, W


class PointEncoderFn(Function):
    """params: W1,b1,g1,be1, ..., W7,b7,g7,be7, W8,b8, fcW, fcb  (32 tensors)."""

    @staticmethod
    def forward(ctx, spec, x, sem, *params):
        x = x.contiguous()
        sem = sem.contiguous()
        M = x.shape[0]
        GR = spec.group_rows
        G = M // GR
        dev = x.device
        W8, b8, fcW, fcb = params[28].reshape(params[28].shape[0], -1), params[29], params[30], params[31]
        S = sem.shape[1]
        Ys, states = [], []
        h, pro, st = x, K.PRO_NONE, None
        pool_ws = None

        def fuse_sem(N):   # (1024 + S) -> 1024, then max-pool over each group
            nonlocal pool_ws
            kin = Ys[4].shape[1]
            kw = dict(group_rows=GR)
            if GR % K.BM == 0:   # pooling partials fused into the GEMM epilogue
                pool_ws = torch.empty(K.nblocks(M), 4, N, device=dev)
                kw.update(pool_ws=pool_ws)
            if spec.mode == "src":   # per-group semantics: a row bias
                W6 = params[20].reshape(N, -1)
                rb = torch.empty(G, N, device=dev)
                K.gemm(G, N, S, sem, S, W6, W6.shape[1], rb, N, B_off=kin)
                kw.update(rowbias=rb, ldr=N)
            else:                    # per-point semantics: further K columns
                kw.update(A2=sem, lda2=S, k1=kin)
            return kw

        for i in range(7):
            kin = h.shape[1]
            Kdim = kin + S if i == 5 and spec.mode == "tgt" else kin
            h, st = _layer_fwd(i, params, h, Kdim, pro, st, spec.bn_modules[i], spec.training, spec.rw, eps=spec.eps,
                               special=fuse_sem if i == 5 else None)
            Ys.append(h)
            states.append(st)
            pro = K.PRO_ENC
        kin = h.shape[1]
        C = W8.shape[0]
        pp = torch.empty(M, C, device=dev)
        K.gemm(M, C, kin, h, kin, W8, W8.shape[1], pp, C, pro_a=K.PRO_ENC, pro_s=st.scale, pro_t=st.shift, bias=b8)
        if pool_ws is not None:
            pooled, argidx = K.pool_finalize(pool_ws, M, Ys[5].shape[1], GR, states[5].scale, states[5].shift)
        else:
            pooled, argidx = K.pool_rows(Ys[5], GR, states[5].scale, states[5].shift)
        code = torch.empty(G, C, device=dev)
        K.gemm(G, C, pooled.shape[1], pooled, pooled.shape[1], fcW, fcW.shape[1], code, C, bias=fcb)
        ctx.spec = spec
        ctx.states = states
        if spec.record is not None:      # diagnostics / parity tests: the max-pool winners and the
            spec.record["pool_rows"] = argidx        # values they were chosen from (relu(Y*scale+shift))
            spec.record["pool_y"], spec.record["pool_scale"], spec.record["pool_shift"] = \
                Ys[5], states[5].scale, states[5].shift
        ctx.save_for_backward(x, sem, pooled, argidx, *Ys, *params)
        return code, pp

    @staticmethod
    def backward(ctx, dcode, dpp):
        spec, states = ctx.spec, ctx.states
        _require_training(spec, "PointEncoderFn")
        saved = ctx.saved_tensors
        x, sem, pooled, argidx = saved[:4]
        Ys = list(saved[4:11])
        params = saved[11:]
        M = x.shape[0]
        GR = spec.group_rows
        G = M // GR
        dev = x.device
        W8, fcW = params[28].reshape(params[28].shape[0], -1), params[30]
        C = W8.shape[0]
        grads = [None] * 32
        bias = _BiasSums()
        dcode = torch.zeros(G, C, device=dev) if dcode is None else dcode.contiguous()
        dpp = torch.zeros(M, C, device=dev) if dpp is None else dpp.contiguous()
        # fc: code = pooled @ fcW^T + fcb
        NP = pooled.shape[1]
        dpool = torch.empty(G, NP, device=dev)
        K.gemm(G, NP, C, dcode, C, fcW, NP, dpool, NP, b_kmajor=True)
        dfcW, dfcb = grad_buffer(fcW), grad_buffer(params[31])
        K.wgrad(dcode, C, pooled, NP, C, NP, G, dfcW, NP)
        K.colsum(dcode, out=dfcb)
        grads[30], grads[31] = dfcW, dfcb
        # per_point_out.3 (no BN): dW8 = dpp^T @ H7
        dW8, db8 = grad_buffer(params[28]).view(W8.shape), grad_buffer(params[29])
        K.wgrad(dpp, C, Ys[6], Ys[6].shape[1], C, W8.shape[1], M, dW8, W8.shape[1],
                pro=K.PRO_ENC, pro_s=states[6].scale, pro_t=states[6].shift)
        K.colsum(dpp, out=db8)
        grads[28], grads[29] = dW8.view(params[28].shape), db8

        def sem_wgrad(dYi, cs, dW):   # semantic columns of fuse_sem
            N, S, kin = dYi.shape[1], sem.shape[1], Ys[4].shape[1]
            if spec.mode == "src":
                # G-row GEMM on the per-group sums: short work
                K.wgrad(_group_sums(dYi, cs, N, G, GR), N, sem, S, N, S, G, dW, dW.shape[1], out_off=kin)
            else:
                K.wgrad(dYi, N, sem, S, N, S, M, dW, dW.shape[1], out_off=kin)

        dY, Wn = dpp, W8   # gradient at the output of the layer above, and that layer's weight
        for i in range(6, -1, -1):
            kw = dict(pool_idx=argidx, pool_grad=dpool, pool_group_rows=GR, special=sem_wgrad) if i == 5 else {}
            dY, Wn = _layer_bwd(i, params, grads, bias, x, Ys, states, dY, Wn, K.ACT_ENC, K.PRO_ENC, spec.rw, **kw)
        bias.flush()
        return (None, None, None) + tuple(grads)


class _BiasSums:
    """Conv-bias gradients of a chain backward: the column sums of each BN layer's per-128-row
    partials of dY (cs [M/128, N], from the BN-backward apply), collected and issued at the end of
    the backward as column-sum jobs of batched node-GEMM launches (csrc/node.hip, up to 6 per
    launch) instead of one launch per layer. Nothing reads them before the optimizer."""

    def __init__(self):
        self.jobs = []

    def add(self, cs, out):
        self.jobs.append((cs, out))
        return out

    def flush(self):
        if self.jobs:
            node.launch(*[node.colsum_desc(cs, out) for cs, out in self.jobs])
        self.jobs = []


def _group_sums(dY, cs, N, G, group_rows):
    """Per-group column sums of dY [G*group_rows, N]. When groups are whole 128-row blocks they
    come from the BN-backward apply's per-block partials cs [M/128, N] (8 MB instead of
    re-reading the 1 GB gradient)."""
    if group_rows % K.BM == 0:
        return K.group_colsum(cs, N, G, group_rows=group_rows // K.BM)
    return K.group_colsum(dY, N, G, group_rows=group_rows)


class ResidualSpec(NamedTuple):
    """Static description of one ResidualNetFn call.

    code_first: True when the input is cat(code, pp) (recon_decoder_src)
    grouping: gidx int32 [M] (row -> group) + off int32 [G+1], or fixed group_rows
    bn_modules: the 3 BatchNorm1d modules (running stats updated in place when training)
    rw: optional K.RowWeights (fixed group_rows only), as in EncoderSpec
    """
    code_first: bool
    gidx: Any
    off: Any
    group_rows: int
    training: bool
    bn_modules: Any
    rw: Any = None


class ResidualNetFn(Function):
    """re_residual_net on cat(per-point pp [M,Cp], group code [G,Cc]); spec: ResidualSpec.

    params: W1,b1,g1,be1, W2,b2,g2,be2, W3,b3,g3,be3, W4,b4 (14 tensors).
    """

    @staticmethod
    def forward(ctx, spec, pp, code, *params):
        pp = pp.contiguous()
        code = code.contiguous()
        M, Cp = pp.shape
        G, Cc = code.shape
        dev = pp.device
        W1 = params[0].reshape(params[0].shape[0], -1)
        ld1 = W1.shape[1]
        assert ld1 == Cp + Cc
        pp_off, code_off = (Cc, 0) if spec.code_first else (0, Cp)
        N1 = W1.shape[0]
        rb = None
        if Cc > 0:   # the group half of the concatenated input becomes a per-group row bias
            rb = torch.empty(G, N1, device=dev)
            K.gemm(G, N1, Cc, code, Cc, W1, ld1, rb, N1, B_off=code_off)

        def first(N):   # the pp columns of W1, the code half as the row bias
            kw = dict(B_off=pp_off)
            if rb is not None:
                kw.update(rowbias=rb, ldr=N1, gidx=spec.gidx, group_rows=spec.group_rows)
            return kw

        Ys, states = [], []
        h, pro, st = pp, K.PRO_NONE, None
        for i in range(3):
            h, st = _layer_fwd(i, params, h, h.shape[1], pro, st, spec.bn_modules[i], spec.training, spec.rw,
                               stat_relu=True, special=first if i == 0 else None)
            Ys.append(h)
            states.append(st)
            pro = K.PRO_RES
        kin = h.shape[1]
        W4 = params[12].reshape(params[12].shape[0], -1)
        out = torch.empty(M, W4.shape[0], device=dev)
        K.gemm(M, W4.shape[0], kin, h, kin, W4, W4.shape[1], out, W4.shape[0], pro_a=K.PRO_RES,
               pro_s=st.scale, pro_t=st.shift, bias=params[13])
        ctx.spec, ctx.states = spec, states
        ctx.save_for_backward(pp, code, *Ys, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        spec, states = ctx.spec, ctx.states
        _require_training(spec, "ResidualNetFn")
        saved = ctx.saved_tensors
        pp, code = saved[:2]
        Ys = list(saved[2:5])
        params = saved[5:]
        M, Cp = pp.shape
        G, Cc = code.shape
        dev = pp.device
        grads = [None] * 14
        bias = _BiasSums()
        dout = dout.contiguous()
        W4 = params[12].reshape(params[12].shape[0], -1)
        No = W4.shape[0]
        dW4, db4 = grad_buffer(params[12]).view(W4.shape), grad_buffer(params[13])
        K.wgrad(dout, No, Ys[2], Ys[2].shape[1], No, W4.shape[1], M, dW4, W4.shape[1],
                pro=K.PRO_RES, pro_s=states[2].scale, pro_t=states[2].shift)
        K.colsum(dout, out=db4)
        grads[12], grads[13] = dW4.view(params[12].shape), db4
        dY, Wn = dout, W4
        W1 = params[0].reshape(params[0].shape[0], -1)
        ld1 = W1.shape[1]
        pp_off, code_off = (Cc, 0) if spec.code_first else (0, Cp)
        dcode = torch.zeros(G, Cc, device=dev)

        def code_half(dYi, cs, dW):   # G-row work on the per-group sums: short kernels
            if Cc == 0:
                return
            N = dYi.shape[1]
            if spec.off is not None:
                D = K.group_colsum(dYi, N, G, off=spec.off)
            else:
                D = _group_sums(dYi, cs, N, G, spec.group_rows)
            K.wgrad(D, N, code, Cc, N, Cc, G, dW, ld1, out_off=code_off)
            # dcode = D @ W1[:, code cols]
            K.gemm(G, Cc, N, D, N, W1, ld1, dcode, Cc, b_kmajor=True, B_off=code_off)

        for i in range(2, -1, -1):
            kw = dict(out_off=pp_off, special=code_half) if i == 0 else {}
            dY, Wn = _layer_bwd(i, params, grads, bias, pp, Ys, states, dY, Wn, K.ACT_RES, K.PRO_RES, spec.rw, **kw)
        bias.flush()
        # input gradient dpp = dY1 @ W1[:, pp cols]
        dpp = torch.empty(M, Cp, device=dev)
        K.gemm(M, Cp, W1.shape[0], dY, W1.shape[0], W1, ld1, dpp, Cp, b_kmajor=True, B_off=pp_off)
        return (None, dpp, dcode) + tuple(grads)


class ChainSpec:
    """Static description of one PointChainFn call (a PointNet conv chain).

    acts: per layer K.ACT_ENC (Conv->BN->ReLU) or K.ACT_BN (Conv->BN; last layer only)
    group_rows: points per cloud (the max-pool groups)
    pool: max-pool the last layer's activation over each group -> pooled [G, N_L]
    want_act: also return the last layer's activation materialised [M, N_L]
    bn_modules: the BatchNorm1d modules (running stats updated in place when training)
    """

    def __init__(self, acts, group_rows, training, bn_modules, pool=True, want_act=False):
        assert all(a == K.ACT_ENC for a in acts[:-1]), "inner layers feed a GEMM prologue: Conv->BN->ReLU only"
        self.acts, self.group_rows, self.training = list(acts), int(group_rows), training
        self.bn_modules, self.pool, self.want_act = bn_modules, pool, want_act


class PointChainFn(Function):
    """Conv1d(k=1)+BatchNorm1d(+ReLU) x L on point-major x [M, Cin], then max-pool over groups of
    spec.group_rows points and/or the last activation (PointNet STN3d / STNkd / PointNetEncoder
    conv stacks, network/pointnet/pointnet_utils.py:27-33,62-68,109-127).

    params: W1,b1,g1,be1, ..., WL,bL,gL,beL. Returns (pooled [G, N_L], act [M, N_L]); an output
    not asked for is an empty tensor. Backward: the last layer's gradient (scattered pool
    gradient + act gradient) enters through a K = 0 BN-backward epilogue; every layer below is
    the fused dgrad + BN-backward GEMM of PointEncoderFn; dx = dY1 @ W1.
    """

    @staticmethod
    def forward(ctx, spec, x, *params):
        _lib.require_device(x, *params)
        x = x.contiguous()
        M = x.shape[0]
        GR = spec.group_rows
        L = len(spec.acts)
        dev = x.device
        Ys, states = [], []
        h, pro, st = x, K.PRO_NONE, None
        pool_ws = None

        def fused_pool(N):   # pooling partials fused into the last GEMM's epilogue
            nonlocal pool_ws
            pool_ws = torch.empty(K.nblocks(M), 4, N, device=dev)
            return dict(pool_ws=pool_ws, group_rows=GR)

        for i in range(L):
            fuse = i == L - 1 and spec.pool and GR % K.BM == 0
            h, st = _layer_fwd(i, params, h, h.shape[1], pro, st, spec.bn_modules[i], spec.training, None,
                               special=fused_pool if fuse else None)
            Ys.append(h)
            states.append(st)
            pro = K.PRO_ENC
        relu_last = spec.acts[-1] == K.ACT_ENC
        NL = Ys[-1].shape[1]
        pooled = argidx = None
        if spec.pool:
            if pool_ws is not None:
                pooled, argidx = K.pool_finalize(pool_ws, M, NL, GR, st.scale, st.shift, relu=relu_last)
            else:
                pooled, argidx = K.pool_rows(Ys[-1], GR, st.scale, st.shift, relu=relu_last)
        act = K.bn_act(Ys[-1], st, relu=relu_last) if spec.want_act else None
        ctx.spec, ctx.states = spec, states
        ctx.save_for_backward(x, argidx, *Ys, *params)
        empty = x.new_empty(0)
        out_p = pooled if pooled is not None else empty
        out_a = act if act is not None else x.new_empty(0)
        if pooled is None:
            ctx.mark_non_differentiable(out_p)
        if act is None:
            ctx.mark_non_differentiable(out_a)
        return out_p, out_a

    @staticmethod
    def backward(ctx, dpooled, dact):
        spec, states = ctx.spec, ctx.states
        _require_training(spec, "PointChainFn")
        saved = ctx.saved_tensors
        L = len(spec.acts)
        x, argidx = saved[0], saved[1]
        Ys = list(saved[2:2 + L])
        params = saved[2 + L:]
        M, Cin = x.shape
        GR = spec.group_rows
        dev = x.device
        grads = [None] * (4 * L)
        use_pool = spec.pool and dpooled is not None and dpooled.numel() > 0
        use_act = spec.want_act and dact is not None and dact.numel() > 0
        bias = _BiasSums()
        # no GEMM feeds the last layer: K = 0 (its own Y stands in for both operands), the epilogue
        # adds the pooled gradient at the winning rows and the activation's own gradient, masks,
        # and reduces
        dY = Wn = Ys[-1]
        kw = dict(Kdim=0)
        if use_pool:
            kw.update(pool_idx=argidx, pool_grad=dpooled.contiguous(), pool_group_rows=GR)
        if use_act:
            kw.update(gadd=dact.contiguous(), ldg=dY.shape[1])
        for i in range(L - 1, -1, -1):
            dY, Wn = _layer_bwd(i, params, grads, bias, x, Ys, states, dY, Wn, spec.acts[i], K.PRO_ENC, None, **kw)
            kw = {}
        bias.flush()
        dx = None
        if ctx.needs_input_grad[1]:
            dx = torch.empty(M, Cin, device=dev)
            K.gemm(M, Cin, dY.shape[1], dY, dY.shape[1], Wn, Wn.shape[1], dx, Cin, b_kmajor=True)
        return (None, dx) + tuple(grads)
