"""Drop-in for the reference network/VN/vn_encoder.py (vn_encoder): the rotation-equivariant
VN-DGCNN encoder that returns the (global feature, per-point features [B, latent, N]) pair. Same
constructor arguments, cfg keys (n_knn, pooling, target_latent_dim), module attributes and
state_dict keys, so a reference checkpoint loads with strict=True.

The four graph levels run fused on ured_hip.vn (one kNN per level, in 3, 63, 63 and 126 dimensions;
no [B, 2C, 3, N, k] tensor with mean pooling, one per-edge tensor per level with max pooling), conv5
and std_feature on the per-point form, all in the point-major [B, N, 3, C] layout. The reference
flattens [B, C, 3, N] as c * 3 + k where this layout flattens k * C + c, so per_point_f reads its
weight columns through that permutation and the pooled [B, 3, C] vector is transposed before
linear1. The tail (pools over N, linear1 / bn1 / leaky_relu / linear2) is the reference's torch code.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from network.VN.vn_layers import *  # noqa: F401,F403  (the reference's import)
from network.VN.vn_layers import VNLinearLeakyReLU, VNMaxPool, VNStdFeature, mean_pool
from network.VN.vn_dgcnn_util import get_graph_feature  # noqa: F401
from ured_hip import vn as V
from ured_hip.gcn import GcnLinearFn


def build_trunk(net, cfg, per_point):
    """The layers the two encoders share, under the reference's attribute names."""
    net.conv1 = VNLinearLeakyReLU(2, 64 // 3)
    net.conv2 = VNLinearLeakyReLU(64 // 3 * 2, 64 // 3)
    net.conv3 = VNLinearLeakyReLU(64 // 3 * 2, 128 // 3)
    net.conv4 = VNLinearLeakyReLU(128 // 3 * 2, 256 // 3)
    net.conv5 = VNLinearLeakyReLU(256 // 3 + 128 // 3 + 64 // 3 * 2, 1024 // 3, dim=4, share_nonlinearity=True)
    net.std_feature = VNStdFeature(1024 // 3 * 2, dim=4, normalize_frame=False)
    net.linear1 = nn.Linear((1024 // 3) * 12, 512)
    net.bn1 = nn.BatchNorm1d(512)
    net.linear2 = nn.Linear(512, cfg['target_latent_dim'])
    if per_point:
        net.per_point_f = nn.Linear((1024 // 3) * 6, cfg['target_latent_dim'])
    if cfg['pooling'] == 'max':
        net.pool1 = VNMaxPool(64 // 3)
        net.pool2 = VNMaxPool(64 // 3)
        net.pool3 = VNMaxPool(128 // 3)
        net.pool4 = VNMaxPool(256 // 3)
    elif cfg['pooling'] == 'mean':
        net.pool1 = mean_pool
        net.pool2 = mean_pool
        net.pool3 = mean_pool
        net.pool4 = mean_pool
    else:
        raise ValueError(f"cfg['pooling'] must be 'max' or 'mean', got {cfg['pooling']!r}")


def trunk_rows(net, x):
    """x [B, 3, N] -> the standardised features [B, N, 3, 2 * (1024 // 3)], point-major. If net.decisions
    is a dict, it receives the forward's discrete decisions: 'idx' (4 x int32 [B,N,k]), 'masks' (7 x
    uint8, conv1..conv5, vn1, vn2) and 'slots' (4 x uint8 with max pooling)."""
    if x.dim() != 3 or x.shape[1] != 3:
        raise ValueError(f"{type(net).__name__}: x must be [B, 3, N], got {tuple(x.shape)}")
    B, _, N = x.shape
    feat = x.float().transpose(1, 2).contiguous().view(B, N, 3, 1)
    dec = getattr(net, "decisions", None)
    ri, rm, rs = (dec.setdefault(k, []) for k in ("idx", "masks", "slots")) if isinstance(dec, dict) else (None, None, None)
    levels = []
    for conv, pool in ((net.conv1, net.pool1), (net.conv2, net.pool2), (net.conv3, net.pool3), (net.conv4, net.pool4)):
        idx = V.knn_rows(feat.detach().view(B, N, -1), net.n_knn)       # once per level
        if ri is not None:
            ri.append(idx)
        if pool is mean_pool:
            feat = conv.forward_graph(feat, idx, "mean", rm)
        else:
            feat = pool.forward_rows(conv.forward_graph(feat, idx, "none", rm), rs)
        levels.append(feat)
    y = net.conv5.forward_rows(torch.cat(levels, dim=3), rm)
    y = torch.cat((y, y.mean(dim=1, keepdim=True).expand_as(y)), dim=3)
    return net.std_feature.forward_rows(y, rm)[0]


def global_rows(net, rows):
    """The pooled tail: rows [B, N, 3, C] -> global_f [B, latent]. If net.decisions is a dict, 'npool'
    receives the point that wins each maximum over N (int64 [B, 3, C])."""
    B, N, _, C = rows.shape
    top, arg = rows.max(dim=1)
    if isinstance(getattr(net, "decisions", None), dict):
        net.decisions["npool"] = arg
    # the reference's feature index is c * 3 + k
    x1 = top.transpose(1, 2).reshape(B, 3 * C)
    x2 = rows.mean(dim=1).transpose(1, 2).reshape(B, 3 * C)
    x = torch.cat((x1, x2), 1)
    x = F.leaky_relu(net.bn1(net.linear1(x)), negative_slope=0.2)
    return net.linear2(x)


class vn_encoder(nn.Module):
    def __init__(self, cfg, num_class=40, normal_channel=False):
        super(vn_encoder, self).__init__()
        self.args = cfg
        self.n_knn = cfg['n_knn']
        build_trunk(self, cfg, per_point=True)

    def forward(self, x):
        rows = trunk_rows(self, x)
        B, N, _, C = rows.shape
        L = self.per_point_f.out_features
        w = self.per_point_f.weight.view(L, C, 3).permute(2, 1, 0).reshape(3 * C, L)    # rows k * C + c
        point_feat = GcnLinearFn.apply(rows.view(B * N, 3 * C), w, self.per_point_f.bias).view(B, N, L)
        global_f = global_rows(self, rows)
        return global_f, point_feat.permute(0, 2, 1)
