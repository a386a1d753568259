"""Drop-in for the reference network/VN/vn_layers.py: the Vector-Neuron layers of the VN-DGCNN
encoders with the reference's names, constructor signatures, attributes and state_dict keys
(map_to_feat.weight, map_to_dir.weight, batchnorm.bn.*, vn1 / vn2 / vn_lin), on ured_hip.vn.

forward() of every module takes and returns the reference's layout, [B, C, 3, N, ...]. The kernels
work point-major with the channel innermost, [B, N, 3, C]; the encoders stay in that layout from end
to end through the *_rows methods and the fused graph layer (VNLinearLeakyReLU.forward_graph), so
the permutes of forward() are for callers of single layers only.

Left out: VNLinearAndLeakyReLU (its constructor raises in the reference: super() names another
class), VNLinear and VNLeakyReLU, which only it uses, and VNStdFeature(normalize_frame=True).
"""
import torch
import torch.nn as nn

from ured_hip import vn as V

EPS = 1e-6


def _to_rows(x):
    """[B, C, 3, N...] -> ([B, prod(N...), 3, C] contiguous, the N... sizes)."""
    rest = tuple(x.shape[3:])
    B, C = x.shape[0], x.shape[1]
    rows = x.reshape(B, C, 3, -1).permute(0, 3, 2, 1).contiguous()
    return rows, rest


def _from_rows(rows, rest):
    """[B, prod(N...), 3, C] -> [B, C, 3, N...]."""
    B, _, _, C = rows.shape
    return rows.permute(0, 3, 2, 1).reshape(B, C, 3, *rest)


class VNBatchNorm(nn.Module):
    """Holds the BatchNorm of a VNLinearLeakyReLU (bn: BatchNorm1d for dim 3 / 4, BatchNorm2d for 5),
    which the fused kernels read and update in place. Its own forward is the reference's composition
    on torch ops; no encoder calls it."""

    def __init__(self, num_features, dim):
        super(VNBatchNorm, self).__init__()
        self.dim = dim
        if dim == 3 or dim == 4:
            self.bn = nn.BatchNorm1d(num_features)
        elif dim == 5:
            self.bn = nn.BatchNorm2d(num_features)

    def forward(self, x):
        norm = torch.norm(x, dim=2) + EPS
        norm_bn = self.bn(norm)
        return x / norm.unsqueeze(2) * norm_bn.unsqueeze(2)


class VNLinearLeakyReLU(nn.Module):
    def __init__(self, in_channels, out_channels, dim=5, share_nonlinearity=False, negative_slope=0.2):
        super(VNLinearLeakyReLU, self).__init__()
        if negative_slope != 0.2:
            raise NotImplementedError("VNLinearLeakyReLU: the kernels fix negative_slope at 0.2")
        self.dim = dim
        self.negative_slope = negative_slope
        self.map_to_feat = nn.Linear(in_channels, out_channels, bias=False)
        self.batchnorm = VNBatchNorm(out_channels, dim=dim)
        if share_nonlinearity == True:  # noqa: E712  (the reference's test)
            self.map_to_dir = nn.Linear(in_channels, 1, bias=False)
        else:
            self.map_to_dir = nn.Linear(in_channels, out_channels, bias=False)

    def forward_rows(self, x, record=None):
        """x [B, M, 3, C_in] -> [B, M, 3, C_out]; the BatchNorm runs over all B * M rows per channel.
        record: a list that receives the leaky mask."""
        out, mask = V.vn_point(x, self.map_to_feat.weight, self.map_to_dir.weight, self.batchnorm.bn)
        if record is not None:
            record.append(mask)
        return out

    def forward_graph(self, x, idx, pool="mean", record=None):
        """get_graph_feature + this layer, fused: x [B, N, 3, C_in / 2], idx int32 [B, N, k] ->
        [B, N, 3, C_out] (pool "mean") or the per-edge [B, N, k, 3, C_out] (pool "none")."""
        out, mask = V.vn_edge(x, idx, self.map_to_feat.weight, self.map_to_dir.weight, self.batchnorm.bn, pool)
        if record is not None:
            record.append(mask)
        return out

    def forward(self, x):
        '''
        x: point features of shape [B, N_feat, 3, N_samples, ...]
        '''
        rows, rest = _to_rows(x)
        return _from_rows(self.forward_rows(rows), rest)


class VNMaxPool(nn.Module):
    def __init__(self, in_channels):
        super(VNMaxPool, self).__init__()
        self.map_to_dir = nn.Linear(in_channels, in_channels, bias=False)

    def forward_rows(self, x, record=None):
        """x [B, N, k, 3, C] -> [B, N, 3, C]. record: a list that receives the winning slots."""
        out, slot = V.VnMaxPoolFn.apply(x, self.map_to_dir.weight)
        if record is not None:
            record.append(slot)
        return out

    def forward(self, x):
        '''
        x: point features of shape [B, N_feat, 3, N_samples, k]
        '''
        if x.dim() != 5:
            raise ValueError(f"VNMaxPool: x must be [B, C, 3, N, k], got {tuple(x.shape)}")
        return self.forward_rows(x.permute(0, 3, 4, 2, 1).contiguous()).permute(0, 3, 2, 1)


def mean_pool(x, dim=-1, keepdim=False):
    return x.mean(dim=dim, keepdim=keepdim)


class VNStdFeature(nn.Module):
    def __init__(self, in_channels, dim=4, normalize_frame=False, share_nonlinearity=False, negative_slope=0.2):
        super(VNStdFeature, self).__init__()
        if normalize_frame:
            raise NotImplementedError("VNStdFeature: normalize_frame=True is not implemented (no encoder uses it)")
        self.dim = dim
        self.normalize_frame = normalize_frame
        self.vn1 = VNLinearLeakyReLU(in_channels, in_channels // 2, dim=dim, share_nonlinearity=share_nonlinearity,
                                     negative_slope=negative_slope)
        self.vn2 = VNLinearLeakyReLU(in_channels // 2, in_channels // 4, dim=dim, share_nonlinearity=share_nonlinearity,
                                     negative_slope=negative_slope)
        self.vn_lin = nn.Linear(in_channels // 4, 3, bias=False)

    def forward_rows(self, x, record=None):
        """x [B, M, 3, C] -> (x_std [B, M, 3, C] with x_std[b,m,k,c] = sum_j x[b,m,j,c] z[b,m,j,k], z [B, M, 3, 3])."""
        B, M = x.shape[0], x.shape[1]
        z = self.vn2.forward_rows(self.vn1.forward_rows(x, record), record)
        z = V.VnLinearFn.apply(z.reshape(B * M * 3, z.shape[3]), self.vn_lin.weight).view(B, M, 3, 3)
        return V.VnFrameFn.apply(x, z), z

    def forward(self, x):
        '''
        x: point features of shape [B, N_feat, 3, N_samples, ...]
        '''
        rows, rest = _to_rows(x)
        std, z = self.forward_rows(rows)
        # the reference's z0 is [B, 3 (j), 3 (k), N...]
        return _from_rows(std, rest), z.permute(0, 2, 3, 1).reshape(x.shape[0], 3, 3, *rest)
