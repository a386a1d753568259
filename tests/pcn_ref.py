"""Restatement of the PCN encoder / decoder (Density_aware_Chamfer_Distance/models/pcn.py:13-71) in
torch on the CPU, float64 by default, in the reference's own [B, C, N] layout with the concatenated
operands built. TEST INFRASTRUCTURE ONLY.

Weights and inputs are regenerated from seeds: make_params builds nn.Conv1d / nn.Linear layers in the
reference's construction order under torch.manual_seed, so it draws the numbers the reference's own
modules draw (tests/golden/make_golden_pcn.py asserts this). Every ReLU mask and pool winner can be
forced (`dec`), which is how the GPU's backward is compared: float64 under the GPU's decisions.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SHAPE = dict(B=2, N=48, num_coarse=16, scale=4)       # the golden's shape (num_points 64)
GOLDEN_SEED = 1
ENC_KEYS = [f"encoder.conv{i}.{p}" for i in (1, 2, 3, 4) for p in ("weight", "bias")]
DEC_KEYS = [f"decoder.{l}.{p}" for l in ("fc1", "fc2", "fc3", "conv1", "conv2", "conv3") for p in ("weight", "bias")]
GRAD_CAP = 512


def grad_sub(t):
    """At most GRAD_CAP evenly strided elements of the flattened tensor."""
    flat = t.reshape(-1)
    return flat[::max(1, -(-flat.numel() // GRAD_CAP))]


def gen_grid_up(up_ratio, grid_size=0.2):
    num_x = max(i for i in range(1, int(math.sqrt(up_ratio)) + 2) if up_ratio % i == 0)
    num_y = up_ratio // num_x
    gx = torch.linspace(-grid_size, grid_size, steps=num_x)
    gy = torch.linspace(-grid_size, grid_size, steps=num_y)
    return torch.stack((gx.repeat_interleave(num_y), gy.repeat(num_x)), 0)


def make_params(seed, num_coarse, output_size=1024):
    """float32 state_dict (reference keys) of torch's default initialisation."""
    torch.manual_seed(seed)
    mods = [("encoder.conv1", nn.Conv1d(3, 128, 1)), ("encoder.conv2", nn.Conv1d(128, 256, 1)),
            ("encoder.conv3", nn.Conv1d(512, 512, 1)), ("encoder.conv4", nn.Conv1d(512, output_size, 1)),
            ("decoder.fc1", nn.Linear(1024, 1024)), ("decoder.fc2", nn.Linear(1024, 1024)),
            ("decoder.fc3", nn.Linear(1024, num_coarse * 3)), ("decoder.conv1", nn.Conv1d(1029, 512, 1)),
            ("decoder.conv2", nn.Conv1d(512, 512, 1)), ("decoder.conv3", nn.Conv1d(512, 3, 1))]
    return {f"{n}.{p}": getattr(m, p).detach().clone() for n, m in mods for p in ("weight", "bias")}


def make_input(seed, B, N):
    r = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(r.random((B, 3, N), dtype=np.float32) - np.float32(0.5))


def cotangents(seed, B, num_coarse, num_fine):
    r = np.random.Generator(np.random.PCG64(1000 + seed))
    return (torch.from_numpy(r.standard_normal((B, 3, num_coarse))), torch.from_numpy(r.standard_normal((B, 3, num_fine))))


def _relu(y, dec, key, pre):
    pre[key] = y
    m = (y > 0) if dec is None or key not in dec else dec[key]
    pre[key + "_mask"] = m
    return y * m.to(y.dtype)


def _maxpool(y, dec, key, pre):
    """y [B,C,N] -> [B,C]; the winner is the first maximal point (torch.max), or dec[key] [B,C]."""
    w = y.max(2)[1] if dec is None or key not in dec else dec[key].long()
    pre[key] = w
    return y.gather(2, w.unsqueeze(2)).squeeze(2)


def encoder(P, x, dec=None, pre=None):
    """x [B,3,N] -> feature [B, Co]. pre (a dict) receives the pre-activations Y1..Y4 [B,C,N], the masks
    and the winners win1 / win2 [B,C] (point indices)."""
    pre = {} if pre is None else pre
    B, _, N = x.shape
    h = _relu(F.conv1d(x, P["encoder.conv1.weight"], P["encoder.conv1.bias"]), dec, "Y1", pre)
    y2 = F.conv1d(h, P["encoder.conv2.weight"], P["encoder.conv2.bias"])
    pre["Y2"] = y2
    g = _maxpool(y2, dec, "win1", pre)
    h = torch.cat((y2, g.unsqueeze(2).expand(-1, -1, N)), 1)
    h = _relu(F.conv1d(h, P["encoder.conv3.weight"], P["encoder.conv3.bias"]), dec, "Y3", pre)
    y4 = F.conv1d(h, P["encoder.conv4.weight"], P["encoder.conv4.bias"])
    pre["Y4"] = y4
    return _maxpool(y4, dec, "win2", pre)


def decoder(P, feat, num_coarse, scale, dec=None, pre=None):
    """feature [B,1024] -> (coarse [B,3,num_coarse], fine [B,3,num_coarse*scale])."""
    pre = {} if pre is None else pre
    B = feat.shape[0]
    nf = num_coarse * scale
    c = _relu(F.linear(feat, P["decoder.fc1.weight"], P["decoder.fc1.bias"]), dec, "A1", pre)
    c = _relu(F.linear(c, P["decoder.fc2.weight"], P["decoder.fc2.bias"]), dec, "A2", pre)
    coarse = F.linear(c, P["decoder.fc3.weight"], P["decoder.fc3.bias"]).view(B, 3, num_coarse)
    grid = gen_grid_up(scale, 0.05).to(feat.dtype)
    grid_feat = grid.unsqueeze(0).repeat(B, 1, num_coarse)
    center = coarse.repeat_interleave(scale, dim=2)                  # every coarse point `scale` times in a row
    h = torch.cat((grid_feat, center, feat.unsqueeze(2).expand(-1, -1, nf)), 1)
    h = _relu(F.conv1d(h, P["decoder.conv1.weight"], P["decoder.conv1.bias"]), dec, "D1", pre)
    h = _relu(F.conv1d(h, P["decoder.conv2.weight"], P["decoder.conv2.bias"]), dec, "D2", pre)
    fine = F.conv1d(h, P["decoder.conv3.weight"], P["decoder.conv3.bias"]) + center
    return coarse, fine


def run(P, x, num_coarse, scale, cot=None, dtype=torch.float64, dec=None, feat_in=None, wrt_x=True):
    """The whole network (or, with feat_in, the decoder alone). -> dict: feat, coarse, fine, pre (the
    pre-activations, masks and winners), grads (name -> gradient under the cotangents `cot` =
    (d coarse, d fine), the input's under "x" / "feat")."""
    Pd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in P.items()}
    pre = {}
    if feat_in is None:
        xin = x.detach().to(dtype).requires_grad_(wrt_x)
        feat = encoder(Pd, xin, dec, pre)
        leaf, leaf_name = xin, "x"
    else:
        feat = feat_in.detach().to(dtype).requires_grad_(True)
        leaf, leaf_name = feat, "feat"
    coarse, fine = decoder(Pd, feat, num_coarse, scale, dec, pre)
    out = {"feat": feat.detach(), "coarse": coarse.detach(), "fine": fine.detach(),
           "pre": {k: v.detach() for k, v in pre.items()}, "grads": {}}
    if cot is not None:
        total = (coarse * cot[0].to(dtype)).sum() + (fine * cot[1].to(dtype)).sum()
        names = [k for k in Pd if feat_in is None or k.startswith("decoder.")]
        leaves = [Pd[k] for k in names] + ([leaf] if leaf.requires_grad else [])
        got = torch.autograd.grad(total, leaves)
        out["grads"] = dict(zip(names + [leaf_name], got))
    return out


def run_encoder(P, x, cot=None, dtype=torch.float64, dec=None):
    """The encoder alone under a cotangent on the feature. -> dict feat, pre, grads."""
    Pd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in P.items() if k.startswith("encoder.")}
    xin = x.detach().to(dtype).requires_grad_(True)
    pre = {}
    feat = encoder(Pd, xin, dec, pre)
    out = {"feat": feat.detach(), "pre": {k: v.detach() for k, v in pre.items()}, "grads": {}}
    if cot is not None:
        names = list(Pd)
        got = torch.autograd.grad((feat * cot.to(dtype)).sum(), [Pd[k] for k in names] + [xin])
        out["grads"] = dict(zip(names + ["x"], got))
    return out


def decisions(pre):
    """The decisions of a run, as `dec` of another."""
    d = {k[:-5]: v for k, v in pre.items() if k.endswith("_mask")}
    d.update({k: pre[k] for k in ("win1", "win2") if k in pre})
    return d


def differing_decisions(pa, pb):
    """Per layer: (differing ReLU masks or winners, elements)."""
    out = {}
    for k in pa:
        if k.endswith("_mask") or k.startswith("win"):
            out[k] = (int((pa[k] != pb[k]).sum()), pa[k].numel())
    return out
