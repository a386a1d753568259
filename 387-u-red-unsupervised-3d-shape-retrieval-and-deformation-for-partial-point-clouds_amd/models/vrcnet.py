"""VRCNet (Density_aware_Chamfer_Distance/models/vrcnet.py:15-539) on the HIP Functions of ured_hip.vrc:
SA_module, SK_SA_module, SKN_Res_unit, SA_SKN_Res_encoder, Linear_ResBlock, Folding, MSAP_SKN_decoder and
Model.

Same names, constructor arguments, parameter names and shapes as the reference (the nn.Conv2d /
nn.Linear modules only hold the parameters, Conv2d weights stay [out, in, 1, 1]), so a reference
state_dict loads with strict=True. forward takes and returns the reference's layouts; forward_rows
keeps everything point-major [B*N, C] between layers.

What differs in how it is computed, not in what:
  - conv1 / conv2 / conv3 of an SA_module commute with the neighbour gather, so they are one GEMM per
    point on stacked weights and the attention core (SaFn) gathers projected rows; no [B, C, k, N]
    tensor is built. The ReLU in front of them is the GEMM's prologue.
  - conv1 and conv_res of an SKN_Res_unit read the same input: one GEMM on stacked weights.
  - the global half of conv6 is a per-cloud row bias of the GEMM; the repeat is never built.
  - each level's kNN and FPS run once and are shared by all branches.
nn.Dropout stays torch's own.

The decoder (vrcnet.py:54-86, 293-403): Folding and MSAP_SKN_decoder here, EF_expansion in
chamfer3D/model_utils.py. Folding never builds its [B, G + C + 2, N r] input (row bias + per-point GEMM +
grid table, FoldFn); the decoder's fully connected and 1x1 layers are linear_rows, FPS on the predicted
points is ured_hip.group.fps from index 0, the gathers are GroupFn (ordered backward), the score ranking is
a stable descending sort (lowest index first on a tie; the reference's topk leaves ties open) and
F.softplus on the scores stays torch's own.

Model (vrcnet.py:406-539): PCN_encoder on [x; y], the posterior / prior heads, LatentFn (softplus, the
reparameterised samples stacked as the generator's [2B, Z] input, both KL terms: one launch each way),
GaussKernelFn for compute_kernel / mmd_loss, one decoder call on the doubled batch and the four-head loss
mix. forward returns what the reference returns. Decided here where the reference leaves a gap or fails:
  - `noise` (keyword only): the standard-normal draws as a sequence of [B, size_z] tensors, consumed in the
    reference's order (training: eps_q, eps_p, then for MMD eps_m, eps_q', eps_p', eps_pfix; evaluation:
    one). None draws them with torch.randn on the input's device.
  - `alpha=None` in training raises ValueError (the reference fails on a NoneType product).
  - `mmd_loss2` exists nowhere in the reference, so its distribution_loss='MMD' branch raises
    AttributeError (every shipped cfg uses KLD); here both MMD terms use mmd_loss.
  - loss='emd': loss4 is the per-cloud emd [2B], as in models/pcn.py; so is the evaluation dict's 'emd'.
  - torch.distributions.Normal's argument validation is not reproduced: a softplus that underflows to 0
    gives an infinite KL here where the reference raises.
  - the reference's Linear_ResBlock rectifies its input in place, so after the heads have run the code that
    goes to the decoder is relu(feat_x) + generator(z) (its in-place ReLU on a chunk of the encoder's output
    is an error in current torch; the rectified value is what it computed where it ran). Stated here with an
    explicit ReLU; the caller's tensors are left as they are.
  - shared fourth head: when the decoder returns `fine` as the very same cloud as `coarse` (num_coarse ==
    num_fine, the shape of vrc_dcd.yaml and vrc_plus.yaml) and loss is cd or dcd, heads 3 and 4 are one
    computation: one calc_cd / calc_dcd call, used as (1 + alpha) * loss.mean(); loss4 is that call's.
  - `pts_num` (getattr(args, "pts_num", None)) is handed to the decoder, for test sizes.

Setting `net.decisions = {}` on a module makes its next forward export the discrete decisions: the
kNN / FPS / pooling-neighbour / three-NN indices of the encoder, the pre-activation of every ReLU
('pre': name -> tensor, the mask is pre > 0) and the pool slots; on Model, 'y_fps' (the FPS indices that
pick y from gt), 'feat' (the code handed to the decoder), 'dl_rec' / 'dl_g' and 'dec' (the decoder's own record).
"""
import math

import torch
import torch.nn as nn

from chamfer3D.model_utils import (EF_expansion, calc_cd, calc_dcd, calc_emd, edge_preserve_sampling_rows, gen_grid_up, knn,
                                   three_nn_upsampling)
from models.pcn import PCN_encoder
from ured_hip.group import GroupFn, fps
from ured_hip.vrc import (CMAX, CenterFn, FoldFn, GaussKernelFn, LatentFn, MaxRowsFn, MMAX, ReluFn, RMAX, SaFn, SkMeanFn,
                          SkMixFn, UnpoolFn, latent_check, linear_rows, sa_check)


def _w2(conv):
    return conv.weight.reshape(conv.weight.shape[0], -1)


def _rows(x):
    """[B, C, 1, N] or [B, C, N] -> point-major [B*N, C]."""
    if x.dim() == 4:
        x = x.squeeze(2)
    return x.transpose(1, 2).reshape(-1, x.shape[1])


def _unrows(y, B, N, four=True):
    y = y.view(B, N, -1).transpose(1, 2)
    return y.unsqueeze(2) if four else y


def _note(rec, name, t):
    if rec is not None:
        rec.setdefault("pre", {})[name] = t


class SA_module(nn.Module):
    def __init__(self, in_planes, rel_planes, mid_planes, out_planes, share_planes=8, k=16):
        super().__init__()
        if mid_planes % share_planes:
            raise ValueError(f"SA_module: share_planes {share_planes} must divide mid_planes {mid_planes}")
        if in_planes > CMAX:
            raise ValueError(f"SA_module: in_planes {in_planes} exceeds {CMAX}")
        sa_check("SA_module", 1, k, k, rel_planes, mid_planes, share_planes)
        self.share_planes = share_planes
        self.k = k
        self.conv1 = nn.Conv2d(in_planes, rel_planes, kernel_size=1)
        self.conv2 = nn.Conv2d(in_planes, rel_planes, kernel_size=1)
        self.conv3 = nn.Conv2d(in_planes, mid_planes, kernel_size=1)
        self.conv_w = nn.Sequential(nn.ReLU(inplace=False),
                                    nn.Conv2d(rel_planes * (k + 1), mid_planes // share_planes, kernel_size=1, bias=False),
                                    nn.ReLU(inplace=False),
                                    nn.Conv2d(mid_planes // share_planes, k * mid_planes // share_planes, kernel_size=1))
        self.activation_fn = nn.ReLU(inplace=False)
        self.conv_out = nn.Conv2d(mid_planes, out_planes, kernel_size=1)

    def forward_rows(self, x, idx, rec=None, tag="sa"):
        """x [B*N, C] (the pre-ReLU input), idx int32 [B, N, k] -> [B*N, out_planes]."""
        if idx.dim() != 3 or idx.shape[2] != self.k:
            raise ValueError(f"SA_module: idx must be [B, N, {self.k}], got {tuple(idx.shape)}")
        if idx.dtype != torch.int32:
            raise TypeError(f"SA_module: idx must be int32, got {idx.dtype}")
        if self.k > idx.shape[1]:
            raise ValueError(f"SA_module: k {self.k} exceeds the cloud's {idx.shape[1]} points")
        rel, mid = self.conv1.out_channels, self.conv3.out_channels
        W = torch.cat((_w2(self.conv1), _w2(self.conv2), _w2(self.conv3)), 0)
        b = torch.cat((self.conv1.bias, self.conv2.bias, self.conv3.bias), 0)
        P = linear_rows(x, W, b, relu_in=True)
        got = {} if rec is not None else None
        o = SaFn.apply(P, idx, _w2(self.conv_w[1]), _w2(self.conv_w[3]), self.conv_w[3].bias, rel, mid, self.share_planes,
                       got)
        if rec is not None:
            _note(rec, tag + ".x", x)
            _note(rec, tag + ".P", P)
            _note(rec, tag + ".h", got["h"])
            _note(rec, tag + ".o", got["o"])
        return linear_rows(o, _w2(self.conv_out), self.conv_out.bias) + x

    def forward(self, input):
        x, idx = input
        B, _, _, N = x.shape
        rec = getattr(self, "decisions", None)
        y = self.forward_rows(_rows(x), idx.int(), rec if isinstance(rec, dict) else None)
        return [_unrows(y, B, N), idx]


class Linear_ResBlock(nn.Module):
    def __init__(self, input_size=1024, output_size=256):
        super().__init__()
        self.conv1 = nn.Linear(input_size, input_size)
        self.conv2 = nn.Linear(input_size, output_size)
        self.conv_res = nn.Linear(input_size, output_size)
        self.af = nn.ReLU(inplace=False)

    def forward(self, feature):
        """conv2(relu(conv1(f))) + conv_res(f) with f = relu(feature): the reference's ReLU is in place, so
        its conv_res reads the rectified input too. The caller's tensor is left as it is here."""
        f = self.af(feature)
        return self.conv2(self.af(self.conv1(f))) + self.conv_res(f)


class SK_SA_module(nn.Module):
    def __init__(self, in_planes, rel_planes, mid_planes, out_planes, share_planes=8, k=[10, 20], r=2, L=32):
        super().__init__()
        if not 1 <= len(k) <= MMAX:
            raise ValueError(f"SK_SA_module: {len(k)} neighbourhood sizes, expected 1..{MMAX}")
        self.num_kernels = len(k)
        d = max(int(out_planes / r), L)
        self.sams = nn.ModuleList([SA_module(in_planes, rel_planes, mid_planes, out_planes, share_planes, k[i])
                                   for i in range(len(k))])
        self.fc = nn.Linear(out_planes, d)
        self.fcs = nn.ModuleList([nn.Linear(d, out_planes) for _ in range(len(k))])
        self.softmax = nn.Softmax(dim=1)
        self.af = nn.ReLU(inplace=False)

    def forward_rows(self, x, idxs, B, relu_out=False, rec=None, tag="sk"):
        """x [B*N, C], idxs: one int32 [B, N, k_i] per branch -> [B*N, out_planes]; relu_out applies the
        ReLU that SKN_Res_unit puts right after the selection."""
        assert self.num_kernels == len(idxs)
        ys = [sam.forward_rows(x, idxs[i], rec, f"{tag}.sam{i}") for i, sam in enumerate(self.sams)]
        for i, y in enumerate(ys):
            _note(rec, f"{tag}.fea{i}", y)
        s = SkMeanFn.apply(B, *ys)
        z = self.fc(s)
        a = self.softmax(torch.stack([fc(z) for fc in self.fcs], 1))
        v = SkMixFn.apply(a, relu_out, *ys)
        if relu_out:
            _note(rec, f"{tag}.v", v)
        return v

    def forward(self, input):
        x, idxs = input
        B, _, _, N = x.shape
        rec = getattr(self, "decisions", None)
        v = self.forward_rows(_rows(x), [i.int() for i in idxs], B, False, rec if isinstance(rec, dict) else None)
        return [_unrows(v, B, N), idxs]


class SKN_Res_unit(nn.Module):
    def __init__(self, input_size, output_size, k=[10, 20], layers=1):
        super().__init__()
        self.conv1 = nn.Conv2d(input_size, output_size, 1, bias=False)
        self.sam = self._make_layer(output_size, output_size // 16, output_size // 4, output_size, int(layers), 8, k=k)
        self.conv2 = nn.Conv2d(output_size, output_size, 1, bias=False)
        self.conv_res = nn.Conv2d(input_size, output_size, 1, bias=False)
        self.af = nn.ReLU(inplace=False)

    def _make_layer(self, in_planes, rel_planes, mid_planes, out_planes, blocks, share_planes=8, k=16):
        return nn.Sequential(*[SK_SA_module(in_planes, rel_planes, mid_planes, out_planes, share_planes, k)
                               for _ in range(blocks)])

    def forward_rows(self, feat, idxs, B, rec=None, tag="unit"):
        """feat [B*N, C_in], idxs: one int32 [B, N, k_i] per branch -> [B*N, output_size]."""
        Co = self.conv1.out_channels
        Y = linear_rows(feat, torch.cat((_w2(self.conv1), _w2(self.conv_res)), 0))       # [conv1 | conv_res]
        x, res = Y[:, :Co], Y[:, Co:]
        n = len(self.sam)
        for i, sk in enumerate(self.sam):
            x = sk.forward_rows(x, idxs, B, i == n - 1, rec, f"{tag}.sk{i}")
        if n == 0:
            _note(rec, f"{tag}.x", x)
            x = ReluFn.apply(x)
        return linear_rows(x, _w2(self.conv2)) + res

    def forward(self, feat, idx):
        B, _, _, N = feat.shape
        rec = getattr(self, "decisions", None)
        y = self.forward_rows(_rows(feat), [i.int() for i in idx], B, rec if isinstance(rec, dict) else None)
        return _unrows(y, B, N)


class SA_SKN_Res_encoder(nn.Module):
    def __init__(self, input_size=3, k=[10, 20], pk=16, output_size=64, layers=[2, 2, 2, 2],
                 pts_num=[3072, 1536, 768, 384]):
        super().__init__()
        self.init_channel = 64
        c1 = self.init_channel
        self.sam_res1 = SKN_Res_unit(input_size, c1, k, int(layers[0]))
        c2 = c1 * 2
        self.sam_res2 = SKN_Res_unit(c2, c2, k, int(layers[1]))
        c3 = c2 * 2
        self.sam_res3 = SKN_Res_unit(c3, c3, k, int(layers[2]))
        c4 = c3 * 2
        self.sam_res4 = SKN_Res_unit(c4, c4, k, int(layers[3]))
        self.conv5 = nn.Conv2d(c4, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 1024)
        self.conv6 = nn.Conv2d(c4 + 1024, c4, 1)
        self.conv7 = nn.Conv2d(c3 + c4, c3, 1)
        self.conv8 = nn.Conv2d(c2 + c3, c2, 1)
        self.conv9 = nn.Conv2d(c1 + c2, c1, 1)
        self.conv_out = nn.Conv2d(c1, output_size, 1)
        self.dropout = nn.Dropout()
        self.af = nn.ReLU(inplace=False)
        self.k = k
        self.pk = pk
        self.rate = 2
        self.pts_num = pts_num

    def _knns(self, pts, rec):
        """pts [B, N, 3] -> one int32 [B, N, k_i] per neighbourhood size."""
        out = [knn(pts.transpose(1, 2), ki).int() for ki in self.k]
        if rec is not None:
            rec.setdefault("knn", []).append(out)
        return out

    def _pool(self, x, pts, S, rec):
        """x [B*N, C] (after the ReLU), pts [B, N, 3] -> (rows [B*S, 2C], the S sampled points)."""
        B, N, _ = pts.shape
        rows, slot, p_idx, pn_idx, out_pts = edge_preserve_sampling_rows(x.view(B, N, -1), pts, S, self.pk)
        if rec is not None:
            rec.setdefault("fps", []).append(p_idx)
            rec.setdefault("pn_idx", []).append(pn_idx)
            rec.setdefault("slot", []).append(slot)
        return rows, out_pts

    def _unpool(self, x, src_pts, tgt_pts, skip, rec):
        """x [B*S, D2] on src_pts, skip [B*N, D1] on tgt_pts -> [B*N, D2 + D1]."""
        B, S, _ = src_pts.shape
        N = tgt_pts.shape[1]
        idx, weight = three_nn_upsampling(tgt_pts, src_pts)
        if rec is not None:
            rec.setdefault("three_nn", []).append(idx)
        return UnpoolFn.apply(x.view(B, S, -1), idx, weight, skip.view(B, N, -1))

    def forward_rows(self, features):
        """features [B, C_in, N] (the first three channels are the coordinates) -> rows [B*N, output_size]."""
        if features.dim() != 3 or features.shape[1] < 3:
            raise ValueError(f"SA_SKN_Res_encoder: features must be [B, C >= 3, N], got {tuple(features.shape)}")
        B, _, N = features.shape
        if N != self.pts_num[0]:
            raise ValueError(f"SA_SKN_Res_encoder: {N} points, pts_num[0] is {self.pts_num[0]}")
        rec = getattr(self, "decisions", None)
        rec = rec if isinstance(rec, dict) else None
        X = features.transpose(1, 2).contiguous().view(B * N, -1)
        pts = [features[:, 0:3, :].detach().transpose(1, 2).contiguous()]
        units = (self.sam_res1, self.sam_res2, self.sam_res3, self.sam_res4)
        skips = []
        x = X
        for lv, unit in enumerate(units):
            if lv:
                x, p = self._pool(skips[-1], pts[-1], self.pts_num[lv], rec)
                pts.append(p)
            x = unit.forward_rows(x, self._knns(pts[lv], rec), B, rec, f"res{lv + 1}")
            _note(rec, f"x{lv + 1}", x)
            skips.append(ReluFn.apply(x))
        x1, x2, x3, x4 = skips
        n4 = self.pts_num[3]
        y5 = linear_rows(x4, _w2(self.conv5), self.conv5.bias)
        g, win = MaxRowsFn.apply(y5, n4)
        if rec is not None:
            rec["win"] = win
        a1 = linear_rows(g, self.fc1.weight, self.fc1.bias)
        _note(rec, "fc1", a1)
        a2 = linear_rows(self.dropout(ReluFn.apply(a1)), self.fc2.weight, self.fc2.bias)
        _note(rec, "fc2", a2)
        g = self.dropout(ReluFn.apply(a2))
        W6 = _w2(self.conv6)
        R6 = linear_rows(g, W6[:, :1024])                      # the global half of conv6: a row bias per cloud
        y = linear_rows(x4, W6[:, 1024:], self.conv6.bias, rowbias=R6, group_rows=n4)
        _note(rec, "conv6", y)
        for name, conv, lv, skip in (("conv7", self.conv7, 2, x3), ("conv8", self.conv8, 1, x2), ("conv9", self.conv9, 0, x1)):
            u = self._unpool(ReluFn.apply(y), pts[lv + 1], pts[lv], skip, rec)
            y = linear_rows(u, _w2(conv), conv.bias)
            _note(rec, name, y)
        return linear_rows(y, _w2(self.conv_out), self.conv_out.bias, relu_in=True)

    def forward(self, features):
        B, _, N = features.shape
        return _unrows(self.forward_rows(features), B, N, four=False)


class Folding(nn.Module):
    """Every coarse point becomes step_ratio points: relu(conv([global | point | grid])). The
    [B, G + C + 2, N r] feature tensor is never built: the global columns of conv are a per-cloud row bias,
    the point columns one GEMM per coarse point (U), the grid columns a [r, output_size] table (T), and
    FoldFn computes relu(U[n] + T[s])."""

    def __init__(self, input_size, output_size, step_ratio, global_feature_size=1024, num_models=1):
        super().__init__()
        if num_models != 1:
            raise ValueError(f"Folding: num_models {num_models} is not supported (the reference's configurations use 1)")
        if not 1 <= step_ratio <= RMAX:
            raise ValueError(f"Folding: step_ratio {step_ratio} outside [1, {RMAX}]")
        self.input_size = input_size
        self.output_size = output_size
        self.step_ratio = step_ratio
        self.num_models = num_models
        self.global_feature_size = global_feature_size
        self.conv = nn.Conv1d(input_size + global_feature_size + 2, output_size, 1, bias=True)
        # [r, 2], x slowest: the reference's meshgrid over num_x x num_y points of +-0.2
        self.register_buffer("grid", gen_grid_up(step_ratio, 0.2).t().contiguous(), persistent=False)

    def forward_rows(self, point_rows, global_feat, rec=None, tag="fold"):
        """point_rows [B*N, C], global_feat [B, G] -> [B*N*r, output_size], row n r + s."""
        C, G = self.input_size, self.global_feature_size
        if global_feat.dim() != 2 or global_feat.shape[1] != G:
            raise ValueError(f"Folding: global_feat must be [B, {G}], got {tuple(global_feat.shape)}")
        B = global_feat.shape[0]
        if point_rows.dim() != 2 or point_rows.shape[1] != C or point_rows.shape[0] % B or point_rows.shape[0] < B:
            raise ValueError(f"Folding: point rows must be [B*N, {C}] for B = {B}, got {tuple(point_rows.shape)}")
        N = point_rows.shape[0] // B
        W = self.conv.weight.view(self.output_size, G + C + 2)
        Rb = linear_rows(global_feat, W[:, :G])
        U = linear_rows(point_rows, W[:, G:G + C], self.conv.bias, rowbias=Rb, group_rows=N)
        T = linear_rows(self.grid, W[:, G + C:])
        out = FoldFn.apply(U, T)
        _note(rec, tag, out)
        return out

    def forward(self, point_feat, global_feat):
        B, C, N = point_feat.shape
        rec = getattr(self, "decisions", None)
        y = self.forward_rows(point_feat.transpose(1, 2).reshape(B * N, C), global_feat, rec if isinstance(rec, dict) else None)
        return y.view(B, N * self.step_ratio, self.output_size).transpose(1, 2)


def rank_scores(scores, num):
    """scores [B, M] -> int32 [B, num]: the num highest, descending, the lowest index first on a tie."""
    return torch.sort(scores, dim=1, descending=True, stable=True)[1][:, :num].int()


def _take(rows, B, idx):
    """rows [B*N, C], idx int32 [B, S] -> [B*S, C], with GroupFn's ordered backward."""
    return GroupFn.apply(None, None, rows.view(B, rows.shape[0] // B, -1), idx.unsqueeze(2).contiguous())


class MSAP_SKN_decoder(nn.Module):
    """The coarse-to-fine decoder: a global code and a partial cloud -> (coarse_raw [B, 3, num_coarse_raw],
    coarse_high [B, 3, (num_coarse_raw + n) up_scale], coarse [B, 3, num_coarse], fine [B, 3, num_fine]).
    pts_num (not in the reference) is handed to the encoder; None keeps the reference's sizes.
    The score selection ranks softplus(score) descending with the lowest index first on a tie.
    `decisions = {}` exports: 'enc' (the encoder's own record), 'knn' / 'slot' / 'H' per EF unit, 'fps',
    'topk', 'scores', and 'pre' (name -> the tensor whose sign is a ReLU mask)."""

    def __init__(self, num_coarse_raw, num_fps, num_coarse, num_fine, layers=[2, 2, 2, 2], knn_list=[10, 20], pk=10,
                 points_label=False, local_folding=False, over_scale=1, pts_num=None):
        super().__init__()
        self.num_coarse_raw = num_coarse_raw
        self.num_fps = num_fps
        self.num_coarse = num_coarse
        self.num_fine = num_fine
        self.points_label = points_label
        self.local_folding = local_folding
        self.fc1 = nn.Linear(1024, 1024)
        self.fc2 = nn.Linear(1024, 1024)
        self.fc3 = nn.Linear(1024, num_coarse_raw * 3)
        self.dense_feature_size = 256
        self.expand_feature_size = 64
        self.input_size = 4 if points_label else 3
        self.encoder = SA_SKN_Res_encoder(input_size=self.input_size, k=knn_list, pk=pk, output_size=self.dense_feature_size,
                                          layers=layers, **({} if pts_num is None else {"pts_num": list(pts_num)}))
        self.up_scale = int(math.ceil(num_fine / (num_coarse_raw + 2048))) * over_scale
        if self.up_scale >= 2:
            self.expansion1 = EF_expansion(input_size=self.dense_feature_size, output_size=self.expand_feature_size,
                                           step_ratio=self.up_scale, k=4)
            self.conv_cup1 = nn.Conv1d(self.expand_feature_size, self.expand_feature_size, 1)
        else:
            self.expansion1 = None
            self.conv_cup1 = nn.Conv1d(self.dense_feature_size, self.expand_feature_size, 1)
        self.conv_cup2 = nn.Conv1d(self.expand_feature_size, 3, 1, bias=True)
        self.conv_s1 = nn.Conv1d(self.expand_feature_size, 16, 1, bias=True)
        self.conv_s2 = nn.Conv1d(16, 8, 1, bias=True)
        self.conv_s3 = nn.Conv1d(8, 1, 1, bias=True)
        if self.local_folding:
            self.expansion2 = Folding(input_size=self.expand_feature_size, output_size=self.dense_feature_size,
                                      step_ratio=(num_fine // num_coarse))
        else:
            self.expansion2 = EF_expansion(input_size=self.expand_feature_size, output_size=self.dense_feature_size,
                                           step_ratio=(num_fine // num_coarse), k=4)
        self.conv_f1 = nn.Conv1d(self.dense_feature_size, self.expand_feature_size, 1)
        self.conv_f2 = nn.Conv1d(self.expand_feature_size, 3, 1)
        self.af = nn.ReLU(inplace=False)

    def forward(self, global_feat, point_input):
        if global_feat.dim() != 2 or global_feat.shape[1] != 1024:
            raise ValueError(f"MSAP_SKN_decoder: global_feat must be [B, 1024], got {tuple(global_feat.shape)}")
        B = global_feat.shape[0]
        if point_input.dim() != 3 or point_input.shape[0] != B or point_input.shape[1] != 3:
            raise ValueError(f"MSAP_SKN_decoder: point_input must be [{B}, 3, n], got {tuple(point_input.shape)}")
        rec = getattr(self, "decisions", None)
        rec = rec if isinstance(rec, dict) else None
        ncr = self.num_coarse_raw
        a1 = linear_rows(global_feat, self.fc1.weight, self.fc1.bias)
        a2 = linear_rows(a1, self.fc2.weight, self.fc2.bias, relu_in=True)
        coarse_raw = linear_rows(a2, self.fc3.weight, self.fc3.bias, relu_in=True).view(B, 3, ncr)
        _note(rec, "fc1", a1)
        _note(rec, "fc2", a2)
        org = point_input
        if self.points_label:
            coarse_input = torch.cat((coarse_raw, coarse_raw.new_zeros(B, 1, ncr)), 1)
            org = torch.cat((org, org.new_ones(B, 1, org.shape[2])), 1)
        else:
            coarse_input = coarse_raw
        points = torch.cat((coarse_input, org), 2)
        if rec is not None:
            self.encoder.decisions = {}
        x = self.encoder.forward_rows(points)                                 # [B*N, 256]
        if rec is not None:
            rec["enc"] = self.encoder.decisions
            del self.encoder.decisions
        N = points.shape[2]
        if self.up_scale >= 2:
            x = self.expansion1.forward_rows(x, B, rec, "exp1")
            N *= self.up_scale
        c1 = linear_rows(x, _w2(self.conv_cup1), self.conv_cup1.bias)
        _note(rec, "cup1", c1)
        feat = ReluFn.apply(c1)                                               # coarse_features [B*N, 64]
        high = linear_rows(feat, _w2(self.conv_cup2), self.conv_cup2.bias)    # coarse_high [B*N, 3]
        pts = high
        if N > self.num_fps:
            idx_fps = fps(high.detach().view(B, N, 3), self.num_fps, start=torch.zeros(B, dtype=torch.int32, device=high.device))
            if rec is not None:
                rec["fps"] = idx_fps
            pts, feat = _take(high, B, idx_fps), _take(feat, B, idx_fps)
            N = self.num_fps
        if rec is not None:
            rec["coarse_fps"] = pts
        if N > self.num_coarse:
            with torch.no_grad():                                             # the scores feed the selection only
                s = linear_rows(feat.detach(), _w2(self.conv_s1), self.conv_s1.bias)
                s = linear_rows(s, _w2(self.conv_s2), self.conv_s2.bias, relu_in=True)
                s = linear_rows(s, _w2(self.conv_s3), self.conv_s3.bias, relu_in=True)
                scores = torch.nn.functional.softplus(s).view(B, N)
                idx_scores = rank_scores(scores, self.num_coarse)
            if rec is not None:
                rec["scores"], rec["topk"] = scores, idx_scores
            pts, feat = _take(pts, B, idx_scores), _take(feat, B, idx_scores)
            N = self.num_coarse
        coarse = pts
        if N < self.num_fine:
            n_fine = N * self.expansion2.step_ratio
            if self.local_folding and n_fine != self.num_fine:
                raise ValueError(f"MSAP_SKN_decoder: {N} coarse points x {self.expansion2.step_ratio} is not num_fine "
                                 f"{self.num_fine}")
            if self.local_folding:
                up = self.expansion2.forward_rows(feat, global_feat, rec, "fold")
            else:
                up = self.expansion2.forward_rows(feat, B, rec, "exp2")
            f1 = linear_rows(up, _w2(self.conv_f1), self.conv_f1.bias)
            _note(rec, "f1", f1)
            fine = linear_rows(f1, _w2(self.conv_f2), self.conv_f2.bias, relu_in=True)
            if self.local_folding:
                fine = CenterFn.apply(fine, coarse)
        else:
            if N != self.num_fine:
                raise ValueError(f"MSAP_SKN_decoder: {N} coarse points exceed num_fine {self.num_fine}")
            fine, n_fine = coarse, N
        coarse_out = _unrows(coarse, B, N, four=False)
        fine_out = coarse_out if fine is coarse else _unrows(fine, B, n_fine, four=False)      # one cloud, one object
        return coarse_raw, _unrows(high, B, high.shape[0] // B, four=False), coarse_out, fine_out


class Model(nn.Module):
    """VRCNet: see the module docstring for the contract and for what is decided here."""

    def __init__(self, args, size_z=128, global_feature_size=1024):
        super().__init__()
        layers = [int(i) for i in args.layers.split(',')]
        knn_list = [int(i) for i in args.knn_list.split(',')]
        latent_check("Model", 1, size_z)
        self.size_z = size_z
        self.distribution_loss = args.distribution_loss
        self.train_loss = args.loss
        self.loss_opts = args.loss_opts
        self.eval_emd = args.eval_emd
        self.encoder = PCN_encoder(output_size=global_feature_size)
        self.posterior_infer1 = Linear_ResBlock(input_size=global_feature_size, output_size=global_feature_size)
        self.posterior_infer2 = Linear_ResBlock(input_size=global_feature_size, output_size=size_z * 2)
        self.prior_infer = Linear_ResBlock(input_size=global_feature_size, output_size=size_z * 2)
        self.generator = Linear_ResBlock(input_size=size_z, output_size=global_feature_size)
        self.decoder = MSAP_SKN_decoder(num_fps=args.num_fps, num_fine=args.num_points, num_coarse=args.num_coarse,
                                        num_coarse_raw=args.num_coarse_raw, layers=layers, knn_list=knn_list, pk=args.pk,
                                        local_folding=args.local_folding, points_label=args.points_label,
                                        pts_num=getattr(args, "pts_num", None))

    def compute_kernel(self, x, y):
        return GaussKernelFn.apply(x, y)

    def mmd_loss(self, x, y):
        return self.compute_kernel(x, x).mean() + self.compute_kernel(y, y).mean() - 2 * self.compute_kernel(x, y).mean()

    def _draws(self, noise, B, like):
        """-> a function returning the next standard-normal [B, size_z] tensor."""
        Z = self.size_z
        if noise is None:
            return lambda: torch.randn(B, Z, device=like.device)
        left = list(noise)

        def draw():
            if not left:
                raise ValueError("Model.forward: noise holds fewer tensors than the forward draws")
            t = left.pop(0)
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (B, Z):
                raise ValueError(f"Model.forward: every noise tensor must be float32 [{B}, {Z}]")
            return t.to(like.device)
        return draw

    def forward(self, x, gt, is_training=True, mean_feature=None, alpha=None, test_emd=True, *, noise=None):
        if x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"Model.forward: x must be [B, 3, n], got {tuple(x.shape)}")
        if gt.dim() != 3 or gt.shape[0] != x.shape[0] or gt.shape[2] != 3:
            raise ValueError(f"Model.forward: gt must be [{x.shape[0]}, m, 3], got {tuple(gt.shape)}")
        if is_training and alpha is None:
            raise ValueError("Model.forward: training needs alpha (the weight of the fine loss)")
        B, _, num_input = x.shape
        rec = getattr(self, "decisions", None)
        rec = rec if isinstance(rec, dict) else None
        draw = self._draws(noise, B, x)
        if is_training:
            gt = gt.contiguous()
            y_idx = fps(gt.detach(), num_input, start=torch.zeros(B, dtype=torch.int32, device=gt.device))
            if rec is not None:
                rec["y_fps"] = y_idx
            y = GroupFn.apply(None, None, gt, y_idx.unsqueeze(2).contiguous()).view(B, num_input, 3).transpose(1, 2)
            feat = self.encoder(torch.cat((x, y), 0).contiguous())
            feat_x, feat_y = ReluFn.apply(feat[:B]), feat[B:]
            o_x = self.posterior_infer2(self.posterior_infer1(feat_x))
            o_y = self.prior_infer(feat_y)
            z, kl_rec, kl_g = LatentFn.apply(o_x, o_y, draw(), draw())
            feat = feat_x.repeat(2, 1) + self.generator(z)
            gt = gt.repeat(2, 1, 1)
            x = x.repeat(2, 1, 1)
        else:
            feat = ReluFn.apply(self.encoder(x.contiguous()))
            o_x = self.posterior_infer2(self.posterior_infer1(feat))
            z = LatentFn.apply(o_x, None, draw(), None)[0]
            feat = feat + self.generator(z)
        if rec is not None:
            rec["feat"] = feat
            self.decoder.decisions = {}
        coarse_raw, coarse_high, coarse, fine = self.decoder(feat, x)
        if rec is not None:
            rec["dec"] = self.decoder.decisions
            del self.decoder.decisions
        shared = fine is coarse
        coarse_raw = coarse_raw.transpose(1, 2).contiguous()
        coarse_high = coarse_high.transpose(1, 2).contiguous()
        coarse = coarse.transpose(1, 2).contiguous()
        fine = coarse if shared else fine.transpose(1, 2).contiguous()
        if not is_training:
            if self.eval_emd and test_emd:
                emd, _ = calc_emd(fine, gt, eps=0.004, iterations=3000)
            else:
                emd = torch.ones(1, device=fine.device)
            _, cd_t, f1 = calc_cd(fine, gt, calc_f1=True)
            dcd, _, _ = calc_dcd(fine, gt)
            return {'out1': coarse_raw, 'out2': fine, 'emd': emd, 'dcd': dcd, 'cd_t': cd_t, 'f1': f1}
        if self.distribution_loss == 'MMD':
            z_m = draw()                                                          # N(0, 1).rsample()
            z2 = LatentFn.apply(o_x, o_y, draw(), draw())[0]
            z_p_fix = LatentFn.apply(o_y.detach(), None, draw(), None)[0]
            dl_rec = self.mmd_loss(z_m, z2[B:])
            dl_g = self.mmd_loss(z2[:B], z_p_fix)
        elif self.distribution_loss == 'KLD':
            dl_rec, dl_g = kl_rec, kl_g
        else:
            raise NotImplementedError('Distribution loss is either MMD or KLD')
        if rec is not None:
            rec["dl_rec"], rec["dl_g"] = dl_rec, dl_g
        if self.train_loss == 'cd':
            def head(cloud, first=False):
                return calc_cd(cloud, gt)[0]
        elif self.train_loss == 'dcd':
            t_alpha, n_lambda = self.loss_opts["alpha"], self.loss_opts["lambda"]

            def head(cloud, first=False):
                return calc_dcd(cloud, gt, alpha=t_alpha * 2 if first else t_alpha, n_lambda=n_lambda)[0]
        elif self.train_loss == 'emd':
            def head(cloud, first=False):
                return calc_cd(cloud, gt)[0]
            shared = False
        else:
            raise NotImplementedError(self.train_loss)
        loss1, loss2 = head(coarse_raw, True), head(coarse_high)
        total_train_loss = loss1.mean() * 10 + loss2.mean() * 0.5
        if shared:
            loss4 = head(coarse)
            total_train_loss = total_train_loss + loss4.mean() * (1 + alpha)
        else:
            loss3 = head(coarse)
            loss4 = calc_emd(fine, gt)[0] if self.train_loss == 'emd' else head(fine)
            total_train_loss = total_train_loss + loss3.mean() + loss4.mean() * alpha
        total_train_loss = total_train_loss + (dl_rec.mean() + dl_g.mean()) * 20
        return fine, loss4, total_train_loss, None
