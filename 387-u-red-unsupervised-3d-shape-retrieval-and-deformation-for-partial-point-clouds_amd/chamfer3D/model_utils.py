"""Drop-in for calc_cd / calc_dcd / calc_emd / fscore (Density_aware_Chamfer_Distance/utils_v2/model_utils.py:13-76,
utils_v2/metrics/CD/fscore.py) on the HIP nearest-neighbour kernels, and gen_grid_up
(Density_aware_Chamfer_Distance/utils/model_utils.py:251-264), and the geometric helpers of VRCNet's encoder
(knn, knn_point, get_edge_features, edge_preserve_sampling, three_nn_upsampling; utils/model_utils.py:200-236,
353-370, 397-404) on the HIP search, sampling and pooling kernels, and the decoder's EF_expansion with
get_graph_feature (utils/model_utils.py:137-166, 267-289) on the edge kernels of ured_hip.vrc.

Note the reference's argument order: calc_cd(output, gt) evaluates cham_loss(gt, output), so
dist1 is gt -> output (model_utils.py:56); kept here.
"""
import math

import torch

from ured_hip import nn as unn
from ured_hip.dcd import DcdLossFn

from .dist_chamfer_3D import chamfer_3DDist


def fscore(dist1, dist2, threshold=0.0001):
    precision_1 = torch.mean((dist1 < threshold).float(), dim=1)
    precision_2 = torch.mean((dist2 < threshold).float(), dim=1)
    f = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
    f[torch.isnan(f)] = 0
    return f, precision_1, precision_2


def calc_cd(output, gt, calc_f1=False, return_raw=False, normalize=False, separate=False):
    dist1, dist2, idx1, idx2 = chamfer_3DDist()(gt, output)
    cd_p = (torch.sqrt(dist1).mean(1) + torch.sqrt(dist2).mean(1)) / 2
    cd_t = dist1.mean(1) + dist2.mean(1)
    if separate:
        res = [torch.cat([torch.sqrt(dist1).mean(1).unsqueeze(0), torch.sqrt(dist2).mean(1).unsqueeze(0)]),
               torch.cat([dist1.mean(1).unsqueeze(0), dist2.mean(1).unsqueeze(0)])]
    else:
        res = [cd_p, cd_t]
    if calc_f1:
        res.append(fscore(dist1, dist2)[0])
    if return_raw:
        res.extend([dist1, dist2, idx1, idx2])
    return res


def calc_dcd(x, gt, alpha=1000, n_lambda=1, return_raw=False, non_reg=False):
    """Density-aware chamfer: 1 - exp(-alpha d) weighted by 1/(visit count of the NN) (model_utils.py:13-51)."""
    x, gt = x.float(), gt.float()
    n_x, n_gt = x.shape[1], gt.shape[1]
    if non_reg:
        frac_12, frac_21 = max(1, n_x / n_gt), max(1, n_gt / n_x)
    else:
        frac_12, frac_21 = n_x / n_gt, n_gt / n_x
    grad = torch.is_grad_enabled() and (x.requires_grad or gt.requires_grad)
    if not grad and n_x + n_gt <= unn.DCD_MAX_POINTS:
        # forward-only (metrics, pseudo-labels): NN + one fused reduction kernel (ured_dcd, or
        # ured_dcd_loss_fwd for a non-integral n_lambda)
        dist1, dist2, idx1, idx2 = unn.nn_dense(gt, x)
        loss, cd_p, cd_t = unn.dcd(dist1, idx1, dist2, idx2, alpha, n_lambda, frac_12, frac_21)
        res = [loss, cd_p, cd_t]
        if return_raw:
            res.extend([dist1, dist2, idx1, idx2])
        return res
    if n_x + n_gt <= unn.DCD_MAX_POINTS:
        # training loss: NN + one reduction launch forward, one launch backward (ured_hip.dcd);
        # cd_p / cd_t stay differentiable through dist1 / dist2 with the torch ops of calc_cd
        loss, dist1, dist2, idx1, idx2 = DcdLossFn.apply(x, gt, alpha, n_lambda, frac_12, frac_21)
        cd_p = (torch.sqrt(dist1).mean(1) + torch.sqrt(dist2).mean(1)) / 2
        cd_t = dist1.mean(1) + dist2.mean(1)
        res = [loss, cd_p, cd_t]
        if return_raw:
            res.extend([dist1, dist2, idx1, idx2])
        return res
    # more than DCD_MAX_POINTS points per pair: the torch tail on the NN Function
    cd_p, cd_t, dist1, dist2, idx1, idx2 = calc_cd(x, gt, return_raw=True)
    # dist1/idx1: every gt point -> its NN in x; dist2/idx2: every x point -> its NN in gt
    exp1, exp2 = torch.exp(-dist1 * alpha), torch.exp(-dist2 * alpha)
    cnt1 = torch.zeros_like(idx2).scatter_add_(1, idx1.long(), torch.ones_like(idx1))
    w1 = (cnt1.gather(1, idx1.long()).float().detach() ** n_lambda + 1e-6) ** (-1) * frac_21
    loss1 = (1 - exp1 * w1).mean(dim=1)
    cnt2 = torch.zeros_like(idx1).scatter_add_(1, idx2.long(), torch.ones_like(idx2))
    w2 = (cnt2.gather(1, idx2.long()).float().detach() ** n_lambda + 1e-6) ** (-1) * frac_12
    loss2 = (1 - exp2 * w2).mean(dim=1)
    res = [(loss1 + loss2) / 2, cd_p, cd_t]
    if return_raw:
        res.extend([dist1, dist2, idx1, idx2])
    return res


def gen_grid_up(up_ratio, grid_size=0.2):
    """The [2, up_ratio] folding grid of the PCN decoder (Density_aware_Chamfer_Distance/utils/
    model_utils.py:251-264): up_ratio = num_x * num_y with num_x the largest divisor not above
    floor(sqrt(up_ratio)) + 1, num_x x num_y points evenly spaced over [-grid_size, grid_size]^2, the
    x coordinate varying slowest."""
    up_ratio = int(up_ratio)
    if up_ratio < 1:
        raise ValueError(f"gen_grid_up: up_ratio must be at least 1, got {up_ratio}")
    num_x = max(i for i in range(1, math.isqrt(up_ratio) + 2) if up_ratio % i == 0)
    num_y = up_ratio // num_x
    gx = torch.linspace(-grid_size, grid_size, steps=num_x)
    gy = torch.linspace(-grid_size, grid_size, steps=num_y)
    return torch.stack((gx.repeat_interleave(num_y), gy.repeat(num_x)), 0).contiguous()


def calc_emd(output, gt, eps=0.005, iterations=50):
    """utils_v2/model_utils.py:72-76: auction EMD (emdModule on csrc/emd.hip) ->
    (sqrt(dist).mean(1) [B], dist [B, n])."""
    from emd import emd
    dist, _ = emd()(output, gt, eps, iterations)
    return torch.sqrt(dist).mean(1), dist


# ---------------- VRCNet encoder helpers (utils/model_utils.py:200-236, 353-370, 397-404) ----------------

def knn(x, k):
    """x [B, D, N] -> int64 [B, N, k]: the k points of the same cloud nearest to each point, the point
    itself included, ranked by (direct squared distance, index). D = 3 goes through ured_hip.nn.knn,
    any other D through ured_hip.vn.knn_rows. No gradient."""
    if x.dim() != 3:
        raise ValueError(f"knn: x must be [B, D, N], got {tuple(x.shape)}")
    rows = x.detach().transpose(1, 2).contiguous().float()
    if k > rows.shape[1]:
        raise ValueError(f"knn: k {k} exceeds the cloud's {rows.shape[1]} points")
    if rows.shape[2] == 3:
        return unn.knn(rows, rows, k)[1].long()
    from ured_hip import vn
    return vn.knn_rows(rows, k).long()


def knn_point(pk, point_input, point_output):
    """The pk points of point_input [B, N, 3] nearest to each point of point_output [B, M, 3] ->
    (dist [B, M, pk] the negated squared distance, descending; idx int64 [B, M, pk]), as the
    reference's topk of -d^2. Ties go to the lowest index."""
    if pk > point_input.shape[1]:
        raise ValueError(f"knn_point: pk {pk} exceeds the cloud's {point_input.shape[1]} points")
    d, idx = unn.knn(point_output.detach().float().contiguous(), point_input.detach().float().contiguous(), pk)
    return -d, idx.long()


def get_edge_features(x, idx):
    """x [B, C, 1, N], idx [B, N, k] -> [B, C, k, N], the gathered neighbour features. Kept for parity
    with the reference's interface; the modules of models/vrcnet.py never build this tensor."""
    B, N, k = idx.shape
    rows = x.squeeze(2).transpose(2, 1).contiguous().view(B * N, -1)
    flat = (idx.long() + torch.arange(B, device=idx.device).view(-1, 1, 1) * N).view(-1)
    return rows[flat].view(B, N, k, -1).permute(0, 3, 2, 1)


def edge_preserve_sampling_rows(feat, point_input, num_samples, k=10):
    """The point-major form the encoder uses. feat [B, N, C], point_input [B, N, 3] -> (rows [B*S, 2C], slot
    uint8 [B, S, C], p_idx int32 [B, S], pn_idx int32 [B, S, pk], point_output [B, S, 3]), S = num_samples."""
    from ured_hip import group
    from ured_hip.vrc import EdgePoolFn
    B, N, _ = feat.shape
    pts = point_input.detach().float().contiguous()
    p_idx = group.fps(pts, num_samples, start=torch.zeros(B, dtype=torch.int32, device=pts.device))
    point_output = torch.gather(point_input, 1, p_idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    pn_idx = knn_point(int(min(k, N)), point_input, point_output)[1].int()
    rows, slot = EdgePoolFn.apply(feat, p_idx, pn_idx)
    return rows, slot, p_idx, pn_idx, point_output


def edge_preserve_sampling(feature_input, point_input, num_samples, k=10):
    """feature_input [B, C, N], point_input [B, N, 3] -> (net [B, 2C, num_samples], p_idx int32
    [B, num_samples], pn_idx int32 [B, num_samples, pk], point_output [B, num_samples, 3]): farthest-point
    sampling from index 0, the pk = min(k, N) nearest input points of every sample, and the sample's own
    feature over the channel-wise max of its neighbours' (ured_hip.vrc.EdgePoolFn)."""
    B, C, N = feature_input.shape
    out, _, p_idx, pn_idx, point_output = edge_preserve_sampling_rows(feature_input.transpose(1, 2).contiguous(), point_input,
                                                                      num_samples, k)
    return out.view(B, num_samples, 2 * C).transpose(1, 2), p_idx, pn_idx, point_output


def three_nn_upsampling(target_points, source_points):
    """target [B, N, 3], source [B, S, 3] -> (idx int32 [B, N, K], weight [B, N, K]), K = min(3, S): the K
    nearest source points of every target point in (distance, index) order and
    weight = (1 / dist) / sum(1 / dist) with dist = max(sqrt(d^2), 1e-10). No gradient."""
    K_ = min(3, source_points.shape[1])
    d2, idx = unn.knn(target_points.detach().float().contiguous(), source_points.detach().float().contiguous(), K_)
    dist = torch.sqrt(d2).clamp(min=1e-10)
    inv = 1.0 / dist
    return idx, inv / inv.sum(2, keepdim=True)


# ---------------- VRCNet decoder: edge-feature expansion (utils/model_utils.py:137-166, 267-289) ----------------

def get_graph_feature(x, k=20, minus_center=True):
    """x [B, C, N] -> [B, 2C, N, k]: the point's own feature over its k nearest neighbours' in feature space
    (minus the point's own when minus_center). Kept for parity with the reference's interface; EF_expansion
    never builds this tensor."""
    idx = knn(x, k)
    B, C, N = x.shape
    rows = x.transpose(2, 1).contiguous()
    flat = (idx + torch.arange(B, device=idx.device).view(-1, 1, 1) * N).view(-1)
    feature = rows.view(B * N, -1)[flat].view(B, N, k, C)
    centre = rows.view(B, N, 1, C).expand(-1, -1, k, -1)
    return torch.cat((centre, feature - centre if minus_center else feature), 3).permute(0, 3, 1, 2)


class EF_expansion(torch.nn.Module):
    """Edge-feature expansion: every point becomes step_ratio points. Same constructor, parameter names and
    shapes as the reference (Conv2d weights [out, in, 1, 1]). With idx = knn(x, k) in feature space:
        f1[n, j]  = conv1([x_n | x_idx[n, j]])
        f2[n, j]  = relu(conv2(relu([f1[n, j] | x_n | x_idx[n, j]])))                    [O r]
        out[n r + s] = max_j conv3(f2[n, j][s O : (s + 1) O])
    The centre and neighbour columns of conv1 / conv2 commute with the gather: they are per-point GEMMs on
    stacked weights, and only the O -> O r product of conv2 on relu(f1) and conv3 run per edge
    (ured_hip.vrc.EfEdgeFn / EfMaxFn). forward takes [B, C, N] and returns [B, O, N r]; forward_rows is
    point-major. Setting `decisions = {}` exports the kNN indices, the ReLU layers and the max slots."""

    def __init__(self, input_size, output_size=64, step_ratio=2, k=4):
        super().__init__()
        from ured_hip.vrc import CMAX, KMAX, OMAX, RMAX
        if not 1 <= input_size <= CMAX:
            raise ValueError(f"EF_expansion: input_size {input_size} outside [1, {CMAX}]")
        if not 1 <= output_size <= OMAX:
            raise ValueError(f"EF_expansion: output_size {output_size} outside [1, {OMAX}]")
        if not 1 <= step_ratio <= RMAX:
            raise ValueError(f"EF_expansion: step_ratio {step_ratio} outside [1, {RMAX}]")
        if not 1 <= k <= KMAX:
            raise ValueError(f"EF_expansion: k {k} outside [1, {KMAX}]")
        self.step_ratio = step_ratio
        self.k = k
        self.input_size = input_size
        self.output_size = output_size
        self.conv1 = torch.nn.Conv2d(input_size * 2, output_size, 1)
        self.conv2 = torch.nn.Conv2d(input_size * 2 + output_size, output_size * step_ratio, 1)
        self.conv3 = torch.nn.Conv2d(output_size, output_size, 1)

    def core_rows(self, x, idx, rec=None, tag="ef"):
        """x [B*N, C], idx int32 [B, N, k] (given) -> [B*N*r, O], row n r + s."""
        from ured_hip.vrc import EfEdgeFn, EfMaxFn, linear_rows
        C, O, r = self.input_size, self.output_size, self.step_ratio
        if idx.dim() != 3 or idx.shape[2] != self.k:
            raise ValueError(f"EF_expansion: idx must be [B, N, {self.k}], got {tuple(idx.shape)}")
        if idx.dtype != torch.int32:
            raise TypeError(f"EF_expansion: idx must be int32, got {idx.dtype}")
        B, N, k = idx.shape
        if x.dim() != 2 or x.shape[0] != B * N or x.shape[1] != C:
            raise ValueError(f"EF_expansion: x must be [{B * N}, {C}], got {tuple(x.shape)}")
        W1 = self.conv1.weight.view(O, 2 * C)
        W2 = self.conv2.weight.view(O * r, O + 2 * C)
        zero1, zero2 = torch.zeros_like(self.conv1.bias), torch.zeros_like(self.conv2.bias)
        # [centre | neighbour] halves of conv1 on x and of conv2 on relu(x): one GEMM each, per point
        P1 = linear_rows(x, torch.cat((W1[:, :C], W1[:, C:]), 0), torch.cat((self.conv1.bias, zero1), 0))
        P2 = linear_rows(x, torch.cat((W2[:, O:O + C], W2[:, O + C:]), 0), torch.cat((self.conv2.bias, zero2), 0),
                         relu_in=True)
        got1, got2 = ({}, {}) if rec is not None else (None, None)
        e1 = EfEdgeFn.apply(P1, idx, None, got1)                              # relu(f1) [B*N*k, O]
        f2 = EfEdgeFn.apply(P2, idx, linear_rows(e1, W2[:, :O]), got2)        # [B*N*k, O r]
        H = linear_rows(f2.view(B * N * k * r, O), self.conv3.weight.view(O, O), self.conv3.bias)
        out, slot = EfMaxFn.apply(H, B, N, k, r)
        if rec is not None:
            pre = rec.setdefault("pre", {})
            pre[tag + ".x"], pre[tag + ".f1"], pre[tag + ".f2"] = x, got1["out"], got2["out"]
            rec.setdefault("slot", {})[tag] = slot
            rec.setdefault("H", {})[tag] = H
        return out

    def forward_rows(self, x, B, rec=None, tag="ef"):
        """x [B*N, C] -> [B*N*r, O]; the neighbours are found here, in feature space."""
        if x.dim() != 2 or x.shape[0] % B:
            raise ValueError(f"EF_expansion: {tuple(x.shape)} rows do not split into {B} clouds")
        N = x.shape[0] // B
        idx = knn(x.detach().reshape(B, N, -1).transpose(1, 2), self.k).int()
        if rec is not None:
            rec.setdefault("knn", {})[tag] = idx
        return self.core_rows(x, idx, rec, tag)

    def forward(self, x):
        B, C, N = x.shape
        rec = getattr(self, "decisions", None)
        y = self.forward_rows(x.transpose(1, 2).reshape(B * N, C), B, rec if isinstance(rec, dict) else None)
        return y.view(B, N * self.step_ratio, self.output_size).transpose(1, 2)
