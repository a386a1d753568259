"""Density-aware chamfer as a training loss (calc_dcd under autograd,
Density_aware_Chamfer_Distance/utils_v2/model_utils.py:13-51) on libured_hip.so.

Forward : the NN launch of nn_dense (ured_nn_fwd_ws) plus one reduction launch
          (ured_dcd_loss_fwd) that also stores d loss / d dist per point.
Backward: one launch (ured_dcd_loss_bwd) for both point gradients.
The visit-count weights are detached, as in the reference. Caller's stream, no host
synchronisation, no allocation inside the library: the Function captures into a HIP graph.
"""
import torch
from torch.autograd import Function

from . import _lib
from .nn import DCD_MAX_POINTS, _as_points, _workspace


def fracs(n_x, n_gt, non_reg=False):
    """(frac_12, frac_21) of calc_dcd (model_utils.py:20-25)."""
    if non_reg:
        return max(1, n_x / n_gt), max(1, n_gt / n_x)
    return n_x / n_gt, n_gt / n_x


class DcdLossFn(Function):
    """(x [B,n_x,3], gt [B,n_gt,3], alpha, n_lambda, frac_12, frac_21) ->
    (loss [B], dist1 [B,n_gt], dist2 [B,n_x], idx1 [B,n_gt] i32, idx2 [B,n_x] i32);
    dist1 / idx1: every gt point -> its NN in x, dist2 / idx2: every x point -> its NN in gt."""

    @staticmethod
    def forward(ctx, x, gt, alpha, n_lambda, frac_12, frac_21):
        x = _as_points(x, "x")
        gt = _as_points(gt, "gt")
        _lib.require_device(x, gt)
        if x.dim() != 3 or gt.dim() != 3 or x.shape[0] != gt.shape[0]:
            raise ValueError(f"expected [B,n_x,3] and [B,n_gt,3], got {tuple(x.shape)} {tuple(gt.shape)}")
        if x.device != gt.device:
            raise ValueError(f"x on {x.device}, gt on {gt.device}")
        b, n2, _ = x.shape
        n1 = gt.shape[1]
        if n1 == 0 or n2 == 0:
            raise ValueError("dcd_loss: empty point set")
        # the reduction's limits first: nothing is launched for a pair it cannot take
        if n1 + n2 > DCD_MAX_POINTS:
            raise _lib.UredError(f"dcd_loss: n_x+n_gt={n1 + n2} exceeds {DCD_MAX_POINTS}")
        if not float(n_lambda) >= 0:
            raise _lib.UredError("dcd_loss: n_lambda must be >= 0")
        dev = x.device
        # the differentiable outputs are allocations of their own (see NNDenseFunction); the
        # indices share one, and so do the two coefficient arrays kept for the backward
        loss = torch.empty(b, device=dev, dtype=torch.float32)
        dist1 = torch.empty(b, n1, device=dev, dtype=torch.float32)
        dist2 = torch.empty(b, n2, device=dev, dtype=torch.float32)
        ibuf = torch.empty(b * (n1 + n2), device=dev, dtype=torch.int32)
        idx1, idx2 = ibuf[:b * n1].view(b, n1), ibuf[b * n1:].view(b, n2)
        cbuf = torch.empty(b * (n1 + n2), device=dev, dtype=torch.float32)
        coef1, coef2 = cbuf[:b * n1].view(b, n1), cbuf[b * n1:].view(b, n2)
        st = _lib.stream_of(x)
        if b:
            ws, nbytes = _workspace(b, n1, n2, b * n1, b * n2, 3, dev)
            _lib.call("ured_nn_fwd_ws", _lib.ptr(gt), _lib.ptr(x), b, n1, n2, 3,
                      _lib.ptr(dist1), _lib.ptr(idx1), _lib.ptr(dist2), _lib.ptr(idx2),
                      _lib.ptr(ws), nbytes, st)
        _lib.call("ured_dcd_loss_fwd", _lib.ptr(dist1), _lib.ptr(idx1), _lib.ptr(dist2), _lib.ptr(idx2), b, n1, n2,
                  float(alpha), float(n_lambda), float(frac_12), float(frac_21), _lib.ptr(loss), None, None,
                  _lib.ptr(coef1), _lib.ptr(coef2), st)
        ctx.save_for_backward(x, gt, idx1, idx2, coef1, coef2)
        ctx.mark_non_differentiable(idx1, idx2)
        ctx.set_materialize_grads(False)
        return loss, dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, g_loss, gd1, gd2, _gi1, _gi2):
        x, gt, idx1, idx2, coef1, coef2 = ctx.saved_tensors
        need_x, need_gt = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        b, n2, _ = x.shape
        n1 = gt.shape[1]
        if not (need_x or need_gt):
            return None, None, None, None, None, None
        if b == 0 or (g_loss is None and gd1 is None and gd2 is None):
            return (torch.zeros_like(x) if need_x else None, torch.zeros_like(gt) if need_gt else None,
                    None, None, None, None)
        # every element is written by the kernel (no zero fill)
        g_x = torch.empty_like(x) if need_x else None
        g_gt = torch.empty_like(gt) if need_gt else None
        g_loss, gd1, gd2 = (None if g is None else g.contiguous() for g in (g_loss, gd1, gd2))
        _lib.call("ured_dcd_loss_bwd", _lib.ptr(gt), _lib.ptr(x), _lib.ptr(idx1), _lib.ptr(idx2),
                  _lib.ptr(coef1), _lib.ptr(coef2), _lib.ptr(g_loss), _lib.ptr(gd1), _lib.ptr(gd2), b, n1, n2,
                  _lib.ptr(g_gt), _lib.ptr(g_x), _lib.stream_of(x))
        return g_x, g_gt, None, None, None, None


def dcd_loss(x, gt, alpha=1000, n_lambda=1, non_reg=False):
    """Differentiable density-aware chamfer of x [B,n_x,3] against gt [B,n_gt,3] (float32, on the
    GPU): (loss [B], dist1 [B,n_gt], dist2 [B,n_x], idx1, idx2). loss, dist1 and dist2 are
    differentiable with respect to x and gt; idx1 / idx2 (int32, lowest index on ties) are not.
    n_lambda is any float >= 0; n_x + n_gt <= 16384."""
    frac_12, frac_21 = fracs(x.shape[1], gt.shape[1], non_reg)
    return DcdLossFn.apply(x, gt, alpha, n_lambda, frac_12, frac_21)
