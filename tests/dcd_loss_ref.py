"""Restatement of calc_dcd as a training loss (Density_aware_Chamfer_Distance/utils_v2/
model_utils.py:13-70) in torch on the CPU, float64 by default. TEST INFRASTRUCTURE ONLY.

The nearest-neighbour decisions are an input (idx1 / idx2, from oracle.nn_ref: the tests check the
GPU's indices bit for bit against it, so forward values and gradients are compared under the same
decisions). The squared distances are the direct differences |p - nn(p)|^2, which is what the
chamfer kernels compute and what the reference's expansion |x|^2 + |y|^2 - 2 x.y equals in exact
arithmetic; their gradient is taken by autograd. The visit counts carry no gradient (detached in
the reference, :35,41).

Inputs are regenerated from seeds (make_inputs); tests/golden/dcd_loss.npz holds only seeds and
the reference's outputs (tests/golden/make_golden_dcd_loss.py).
"""
import numpy as np
import torch

# (alpha, n_lambda, non_reg)
PARAMS = [(1000, 1, False), (200, 0.5, False), (50, 0, True), (200, 2, False)]
# golden cases: name -> (seed, B, n_x, n_gt)
GOLDEN_CASES = {"r3x63x65": (11, 3, 63, 65), "r2x300x200": (12, 2, 300, 200)}


def make_inputs(seed, b, n_x, n_gt):
    """x [b,n_x,3] clustered towards the origin (so that visit counts vary), gt [b,n_gt,3] uniform."""
    r = np.random.Generator(np.random.PCG64(seed))
    x = r.random((b, n_x, 3), dtype=np.float32) ** 2
    gt = r.random((b, n_gt, 3), dtype=np.float32)
    return x, gt


def cotangent(b, scale=1.0):
    """A fixed per-item upstream gradient that differs across the batch."""
    return scale * (0.5 + np.arange(b, dtype=np.float64) / max(1, b))


def param_tag(alpha, n_lambda, non_reg):
    return f"a{alpha}l{n_lambda}nr{int(non_reg)}"


def fracs(n_x, n_gt, non_reg):
    if non_reg:
        return max(1, n_x / n_gt), max(1, n_gt / n_x)
    return n_x / n_gt, n_gt / n_x


def forward(x, gt, idx1, idx2, alpha, n_lambda, non_reg=False):
    """x [B,n_x,3], gt [B,n_gt,3] tensors of one dtype; idx1 [B,n_gt] (gt -> x), idx2 [B,n_x]
    (x -> gt) integer tensors. -> dict(loss, cd_p, cd_t, dist1, dist2)."""
    i1, i2 = torch.as_tensor(idx1).long(), torch.as_tensor(idx2).long()
    n_x, n_gt = x.shape[1], gt.shape[1]
    frac_12, frac_21 = fracs(n_x, n_gt, non_reg)
    dist1 = ((torch.gather(x, 1, i1[..., None].expand(-1, -1, 3)) - gt) ** 2).sum(-1)
    dist2 = ((torch.gather(gt, 1, i2[..., None].expand(-1, -1, 3)) - x) ** 2).sum(-1)
    one = torch.ones((), dtype=x.dtype)
    cnt1 = torch.zeros(x.shape[0], n_x, dtype=x.dtype).scatter_add_(1, i1, one.expand(i1.shape))
    cnt2 = torch.zeros(x.shape[0], n_gt, dtype=x.dtype).scatter_add_(1, i2, one.expand(i2.shape))
    w1 = (cnt1.gather(1, i1) ** n_lambda + 1e-6) ** (-1) * frac_21
    w2 = (cnt2.gather(1, i2) ** n_lambda + 1e-6) ** (-1) * frac_12
    loss1 = (1 - torch.exp(-dist1 * alpha) * w1).mean(1)
    loss2 = (1 - torch.exp(-dist2 * alpha) * w2).mean(1)
    return {"loss": (loss1 + loss2) / 2,
            "cd_p": (torch.sqrt(dist1).mean(1) + torch.sqrt(dist2).mean(1)) / 2,
            "cd_t": dist1.mean(1) + dist2.mean(1), "dist1": dist1, "dist2": dist2}


def run(x, gt, idx1, idx2, alpha, n_lambda, non_reg=False, cot=None, dtype=torch.float64, wrt=("x", "gt")):
    """Forward values and, under the cotangents `cot` (name of an output -> array shaped like it),
    the gradients with respect to x and gt. numpy in; -> (dict of detached outputs, dict of grads)."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_("x" in wrt)
    gtt = torch.from_numpy(np.ascontiguousarray(gt)).to(dtype).requires_grad_("gt" in wrt)
    out = forward(xt, gtt, idx1, idx2, alpha, n_lambda, non_reg)
    grads = {}
    if cot:
        total = sum((out[k] * torch.as_tensor(np.asarray(v)).to(dtype)).sum() for k, v in cot.items())
        leaves = [t for t in (xt, gtt) if t.requires_grad]
        got = torch.autograd.grad(total, leaves)
        grads = dict(zip([n for n in ("x", "gt") if n in wrt], got))
    return {k: v.detach() for k, v in out.items()}, grads
