"""Restatement of VRCNet's Model (Density_aware_Chamfer_Distance/models/vrcnet.py:406-539) in torch on the CPU,
float64 by default. TEST INFRASTRUCTURE ONLY.

  latent / gauss / mmd   the latent head (softplus, rsample, the two kl_divergence terms) and compute_kernel /
                         mmd_loss, written with plain torch ops
  model_forward          the heads, the doubled batch and the loss mix, composed from pcn_ref.encoder,
                         vrc_ref.linear_resblock, dcd_loss_ref.forward and a decoder passed in as a function

The golden (tests/golden/vrcmodel.npz, written by tests/golden/make_golden_vrcmodel.py from the reference's own
Model) replaces the decoder by a linear stub, stub_decoder below: each of the four clouds is base_i +
reshape(code @ S_i), so gradient reaches the heads through the losses as well as through the KL terms. Inputs,
weights, the stub and the noise are regenerated from the seed; the npz holds only data.

The reference's Linear_ResBlock rectifies its input in place, so the code handed to the decoder is
relu(feat_x) + generator(z): stated here with an explicit ReLU.

The nearest-neighbour picks of the loss heads and the FPS picks of y are decisions. GOLDEN_SEED is the first seed
below 256 at which, for every combination of COMBOS and both stub variants, every NN argmin gap of the loss
heads is at least MARGIN_MULT = 4 times the forward tolerance (tests/tol_check.py's rule) of its distance
matrix, the FPS steps on gt keep GEO_MARGIN, and float32 makes the same picks. Few seeds do (the heads make about
1400 picks per combination, and 40 of the 256 seeds keep the FPS margin alone): 43 is the first, and only 43
qualifies below 256; its smallest ratio is GOLDEN_RATIO (float32 on another CPU moves it by a percent or so).
"""
import numpy as np
import torch

import dcd_loss_ref
import pcn_ref
import vrc_ref as R
from tol_check import F_FWD, FLOOR_MULT

GOLDEN_SEED = 43
GOLDEN_RATIO = 5.63
MARGIN_MULT = 4.0
GRAD_CAP = 256
ALPHA = 0.5                 # forward's alpha, the weight of the fourth head
FIX = dict(B=2, n_in=40, n_gt=48, clouds=(24, 64, 16, 32), size_z=128, G=1024)
# name -> (loss, distribution_loss, loss_opts)
COMBOS = {"cd_kld": ("cd", "KLD", None), "dcd_kld": ("dcd", "KLD", {"alpha": 40, "lambda": 0.5}), "cd_mmd": ("cd", "MMD", None)}
# the rest of args, for the key list and shapes of the real Model (no loss field)
KEY_ARGS = dict(layers="1,1,1,1", knn_list="4", eval_emd=True, num_fps=16, num_points=32, num_coarse=16, num_coarse_raw=40, pk=4,
                local_folding=True, points_label=False)
HEADS = ("posterior_infer1", "posterior_infer2", "prior_infer", "generator")
CLOUDS = ("coarse_raw", "coarse_high", "coarse", "fine")
GAUSS_SHAPES = [(1, 1, 1), (3, 5, 7), (6, 4, 128)]      # fixed compute_kernel / mmd_loss values in the golden


def grad_sub(t):
    """At most GRAD_CAP evenly strided elements of the flattened tensor."""
    flat = t.reshape(-1)
    return flat[::max(1, -(-flat.numel() // GRAD_CAP))]


def head_sizes(size_z=128, G=1024):
    return {"posterior_infer1": (G, G), "posterior_infer2": (G, 2 * size_z), "prior_infer": (G, 2 * size_z),
            "generator": (size_z, G)}


def make_params(seed, size_z=128, G=1024):
    """float32 state_dict (reference keys) of the encoder and the four heads under torch's default
    initialisation, in the reference's construction order (the decoder is constructed after them)."""
    import torch.nn as nn
    torch.manual_seed(seed)
    mods = [("encoder.conv1", nn.Conv1d(3, 128, 1)), ("encoder.conv2", nn.Conv1d(128, 256, 1)),
            ("encoder.conv3", nn.Conv1d(512, 512, 1)), ("encoder.conv4", nn.Conv1d(512, G, 1))]
    for name, (i, o) in head_sizes(size_z, G).items():
        mods += [(f"{name}.conv1", nn.Linear(i, i)), (f"{name}.conv2", nn.Linear(i, o)), (f"{name}.conv_res", nn.Linear(i, o))]
    return {f"{n}.{p}": getattr(m, p).detach().clone() for n, m in mods for p in ("weight", "bias")}


def make_inputs(seed, B, n_in, n_gt):
    """x [B, 3, n_in] and gt [B, n_gt, 3], float32, uniform in [-0.5, 0.5]^3."""
    r = np.random.Generator(np.random.PCG64(200 + seed))
    x = torch.from_numpy(r.random((B, 3, n_in), dtype=np.float32) - np.float32(0.5))
    gt = torch.from_numpy(r.random((B, n_gt, 3), dtype=np.float32) - np.float32(0.5))
    return x, gt


def make_noise(seed, B, size_z, count=6):
    """The standard-normal draws, float32 [B, size_z] each, in the order forward consumes them."""
    r = np.random.Generator(np.random.PCG64(300 + seed))
    return [torch.from_numpy(r.standard_normal((B, size_z)).astype(np.float32)) for _ in range(count)]


def make_stub(seed, clouds, G=1024):
    """[(base_i [3, n_i], S_i [G, 3 n_i])] float32: cloud_i = base_i + reshape(code @ S_i)."""
    r = np.random.Generator(np.random.PCG64(400 + seed))
    out = []
    for n in clouds:
        base = torch.from_numpy(r.random((3, n), dtype=np.float32) - np.float32(0.5))
        S = torch.from_numpy(r.standard_normal((G, 3 * n)).astype(np.float32) * np.float32(0.05 / np.sqrt(G)))
        out.append((base, S))
    return out


def stub_decoder(stub, code, shared=False):
    """code [R, G] -> the four clouds [R, 3, n_i]; shared: the fourth tensor is returned as coarse and fine."""
    outs = [b.to(code.dtype) + (code @ S.to(code.dtype)).view(code.shape[0], 3, -1) for b, S in stub]
    if shared:
        outs[2] = outs[3]
    return tuple(outs)


# ---------------- the kernels' contracts ----------------

def softplus(x):
    """torch's softplus (beta 1, threshold 20), written out."""
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20))))


def kl_normal(mp, sp, mq, sq):
    """KL(N(mp, sp) || N(mq, sq)) in the form of torch's kl_divergence."""
    r = (sp / sq) ** 2
    t = ((mp - mq) / sq) ** 2
    return 0.5 * (r + t - 1 - torch.log(r))


def latent(oq, op, eps_q, eps_p):
    """-> (z, kl_rec, kl_g); op = eps_p = None gives (z [B, Z], None, None). The prior is detached in kl_g."""
    Z = oq.shape[1] // 2
    mq, sq = oq[:, :Z], softplus(oq[:, Z:])
    zq = mq + sq * eps_q.to(oq.dtype)
    if op is None:
        return zq, None, None
    mp, sp = op[:, :Z], softplus(op[:, Z:])
    zp = mp + sp * eps_p.to(oq.dtype)
    kl_rec = kl_normal(torch.zeros_like(mp), torch.ones_like(sp), mp, sp)
    kl_g = kl_normal(mp.detach(), sp.detach(), mq, sq)
    return torch.cat((zq, zp), 0), kl_rec, kl_g


def gauss(x, y):
    """compute_kernel: exp(-mean_d((x_i - y_j)^2) / Z) [n, m]."""
    return torch.exp(-((x[:, None, :] - y[None, :, :]) ** 2).mean(2) / float(x.shape[1]))


def mmd(x, y):
    return gauss(x, x).mean() + gauss(y, y).mean() - 2 * gauss(x, y).mean()


def gauss_inputs(n, m, Z):
    r = np.random.Generator(np.random.PCG64(500 + 100 * n + 10 * m + Z))
    return (torch.from_numpy(r.standard_normal((n, Z)).astype(np.float32)),
            torch.from_numpy(r.standard_normal((m, Z)).astype(np.float32)))


# ---------------- the model ----------------

def nn_pick(a, b):
    """For every point of a [B, n, 3] its nearest in b [B, m, 3] by the direct squared distance, the lowest index
    on a tie -> (idx [B, n], the smallest gap to the runner-up, the distance matrix)."""
    d = R._d2(a, b)
    idx = d.argmin(2)
    gap = float("inf")
    if b.shape[1] > 1:
        two = d.topk(2, dim=2, largest=False)[0]
        gap = (two[:, :, 1] - two[:, :, 0]).min().item()
    return idx, gap, d


def _sub(P, prefix):
    return {k[len(prefix) + 1:]: v for k, v in P.items() if k.startswith(prefix + ".")}


def _lrb(P, name, x):
    return R.linear_resblock(_sub(P, name), x, R.Dec())


def loss_head(dec, name, cloud, gt, loss, opts, first=False):
    """cloud [R, n, 3], gt [R, m, 3] -> the per-cloud loss [R] of calc_cd (cd_p) or calc_dcd."""
    def pick(tag, a, b):
        def fn():
            idx, gap, d = nn_pick(a.detach(), b.detach())
            dec.pre[f"{name}.{tag}.d"] = d
            return idx, gap
        return dec.pick(f"{name}.{tag}", fn)
    idx1, idx2 = pick("idx1", gt, cloud), pick("idx2", cloud, gt)
    if loss == "dcd":
        return dcd_loss_ref.forward(cloud, gt, idx1, idx2, opts["alpha"] * (2 if first else 1), opts["lambda"])["loss"]
    return dcd_loss_ref.forward(cloud, gt, idx1, idx2, 1, 1)["cd_p"]


def model_forward(P, x, gt, noise, combo, alpha=ALPHA, decoder=None, shared=False, force=None):
    """One training forward. P, x, gt of one dtype; noise float32 tensors; decoder: code [2B, G] -> four clouds
    [2B, 3, n_i]. -> dict: y_fps, feat (the code handed to the decoder), dl_rec, dl_g, loss4, total, fine, and
    dec (vrc_ref.Dec: the picks, their margins, the distance matrices under pre)."""
    loss, dist, opts = COMBOS[combo] if isinstance(combo, str) else combo
    dec = R.Dec(force)
    B, _, n_in = x.shape
    noise = list(noise)
    y_idx = dec.pick("y_fps", lambda: R.fps_pick(gt.detach(), n_in))
    y = torch.gather(gt, 1, y_idx.unsqueeze(-1).expand(-1, -1, 3)).transpose(1, 2)
    feat = pcn_ref.encoder(P, torch.cat((x, y), 0))
    feat_x, feat_y = torch.relu(feat[:B]), feat[B:]
    o_x = _lrb(P, "posterior_infer2", _lrb(P, "posterior_infer1", feat_x))
    o_y = _lrb(P, "prior_infer", feat_y)
    z, kl_rec, kl_g = latent(o_x, o_y, noise.pop(0), noise.pop(0))
    code = torch.cat((feat_x, feat_x), 0) + _lrb(P, "generator", z)
    clouds = decoder(code)
    same = clouds[3] is clouds[2]
    assert same == shared
    clouds = [c.transpose(1, 2) for c in clouds]
    gt2 = torch.cat((gt, gt), 0)
    if dist == "MMD":
        z_m = noise.pop(0).to(x.dtype)
        z2 = latent(o_x, o_y, noise.pop(0), noise.pop(0))[0]
        z_fix = latent(o_y.detach(), None, noise.pop(0), None)[0]
        dl_rec, dl_g = mmd(z_m, z2[B:]), mmd(z2[:B], z_fix)
    else:
        dl_rec, dl_g = kl_rec, kl_g
    l1 = loss_head(dec, "coarse_raw", clouds[0], gt2, loss, opts, True)
    l2 = loss_head(dec, "coarse_high", clouds[1], gt2, loss, opts)
    l3 = loss_head(dec, "coarse", clouds[2], gt2, loss, opts)
    l4 = l3 if same else loss_head(dec, "fine", clouds[3], gt2, loss, opts)
    total = l1.mean() * 10 + l2.mean() * 0.5 + l3.mean() + l4.mean() * alpha + (dl_rec.mean() + dl_g.mean()) * 20
    return {"y_fps": y_idx, "feat": code, "dl_rec": dl_rec, "dl_g": dl_g, "loss4": l4, "total": total, "fine": clouds[3],
            "dec": dec}


def fixture(seed=GOLDEN_SEED):
    """-> (P, x, gt, noise, stub), float32."""
    F_ = FIX
    x, gt = make_inputs(seed, F_["B"], F_["n_in"], F_["n_gt"])
    return (make_params(seed, F_["size_z"], F_["G"]), x, gt, make_noise(seed, F_["B"], F_["size_z"]),
            make_stub(seed, F_["clouds"], F_["G"]))


def run_fixture(combo, dtype=torch.float64, shared=False, seed=GOLDEN_SEED, grads=True, force=None):
    """The fixture through model_forward with the stub decoder -> its dict with detached values, plus grads
    (parameter name -> gradient of total, and "x")."""
    P, x, gt, noise, stub = fixture(seed)
    Pd = {k: v.to(dtype).requires_grad_(True) for k, v in P.items()}
    xd = x.to(dtype).requires_grad_(True)
    out = model_forward(Pd, xd, gt.to(dtype), noise, combo, decoder=lambda c: stub_decoder(stub, c, shared), shared=shared,
                        force=force)
    if grads:
        names = list(Pd)
        got = torch.autograd.grad(out["total"], [Pd[k] for k in names] + [xd])
        out["grads"] = dict(zip(names + ["x"], got))
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def decision_ratio(r64, r32):
    """The smallest NN argmin gap of the loss heads over the forward tolerance of its distance matrix."""
    worst = float("inf")
    d64, d32 = r64["dec"], r32["dec"]
    for k, gap in d64.margin.items():
        if k == "y_fps":
            continue
        a64, a32 = d64.pre[k + ".d"], d32.pre[k + ".d"].double()
        tol = FLOOR_MULT * (a32 - a64).abs().max().item() + F_FWD * a64.abs().max().item()
        worst = min(worst, gap / tol)
    return worst


def qualify(seed):
    """-> the smallest ratio over all combinations and both stub variants, or None when the seed fails the rule."""
    worst = float("inf")
    for combo in COMBOS:
        for shared in (False, True):
            r64 = run_fixture(combo, torch.float64, shared, seed, grads=False)
            r32 = run_fixture(combo, torch.float32, shared, seed, grads=False)
            if r64["dec"].margin["y_fps"] < R.GEO_MARGIN:
                return None
            if any(not torch.equal(v, r32["dec"].idx[k]) for k, v in r64["dec"].idx.items()):
                return None
            worst = min(worst, decision_ratio(r64, r32))
    return worst if worst >= MARGIN_MULT else None
