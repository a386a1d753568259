"""Drop-in for the reference network/pointnet/pointnet2_utils.py (:43-315): index_points,
farthest_point_sample, query_ball_point, sample_and_group, sample_and_group_all,
PointNetSetAbstraction, PointNetSetAbstractionMsg and PointNetFeaturePropagation, with the
reference's names, signatures, [B, C, N] layer convention and state_dict keys, so checkpoints
interchange. The pointnet2_* model files beside this one are built on them.

Farthest-point sampling, the ball query and the grouping (with its backward) are the HIP kernels
of ured_hip.group (csrc/group.hip); the layer's Conv2d(1x1) -> BatchNorm2d -> ReLU stack and its
max over nsample run as ONE fused ured_hip.mlp.PointChainFn call on the point-major
[B*npoint*nsample, C] matrix the grouping kernel writes. Index tensors are torch.long here, as in
the reference; the kernels work in int32.

Distances are d = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32 where the reference's ball query expands
|a|^2 + |b|^2 - 2ab: the two agree bit for bit only where every intermediate is exact.
farthest_point_sample / PointNetSetAbstraction.forward take an optional start= (the reference
draws it with torch.randint) for reproducible sampling; so does PointNetSetAbstractionMsg.forward,
which samples and gathers the centroids once and runs ball query -> grouping -> one fused chain per
scale.

PointNetFeaturePropagation is three_nn (ured_hip.nn.knn, K = min(3, S)) -> InterpFn (csrc/
interp.hip: the inverse-distance weights, the gather, the weighted sum and the cat with the skip
features in one launch) -> one PointChainFn call for its Conv1d -> BatchNorm1d -> ReLU stack. The
neighbour distances are knn's fmaf(dz,dz, fmaf(dy,dy, dx*dx)) where the reference expands
|a|^2 + |b|^2 - 2ab and sorts the whole row.
"""
import torch
import torch.nn as nn

from ured_hip import group as G
from ured_hip import interp as I
from ured_hip import kernels as K
from ured_hip.mlp import ChainSpec, PointChainFn


def index_points(points, idx):
    """points [B,N,C], idx long [B,S] or [B,S,K] -> points[b, idx] [B,S,C] / [B,S,K,C]
    (pointnet2_utils.py:43-60). Differentiable in points; an index outside [0,N) gives zeros."""
    B = idx.shape[0]
    i3 = idx.reshape(B, idx.shape[1], -1).to(torch.int32)
    out = G.GroupFn.apply(None, None, points, i3)
    return out.view(*idx.shape, points.shape[-1])


def farthest_point_sample(xyz, npoint, start=None):
    """xyz [B,N,3] -> centroids long [B,npoint] (pointnet2_utils.py:63-84); start: the first index
    of every cloud (int tensor [B]); None draws it as the reference does."""
    return G.fps(xyz, npoint, start).long()


def query_ball_point(radius, nsample, xyz, new_xyz):
    """-> group_idx long [B,S,nsample] (pointnet2_utils.py:87-107)."""
    return G.ball_query(radius, nsample, xyz, new_xyz).long()


def _sample_and_group(npoint, radius, nsample, xyz, points, start=None):
    """-> new_xyz [B,S,3], the point-major grouped matrix [B*S*nsample, 3+D], idx int32, fps_idx int32."""
    B = xyz.shape[0]
    fps_idx = G.fps(xyz, npoint, start)
    new_xyz = G.GroupFn.apply(None, None, xyz, fps_idx.view(B, npoint, 1)).view(B, npoint, 3)
    idx = G.ball_query(radius, nsample, xyz, new_xyz)
    return new_xyz, G.GroupFn.apply(xyz, new_xyz, points, idx), idx, fps_idx


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, start=None):
    """xyz [B,N,3], points [B,N,D] | None -> new_xyz [B,npoint,3], new_points [B,npoint,nsample,3+D]
    (pointnet2_utils.py:110-138); returnfps adds grouped_xyz [B,npoint,nsample,3] and fps_idx."""
    B = xyz.shape[0]
    new_xyz, rows, idx, fps_idx = _sample_and_group(npoint, radius, nsample, xyz, points, start)
    new_points = rows.view(B, npoint, nsample, -1)
    if returnfps:
        grouped_xyz = G.GroupFn.apply(None, None, xyz, idx).view(B, npoint, nsample, 3)
        return new_xyz, new_points, grouped_xyz, fps_idx.long()
    return new_xyz, new_points


def sample_and_group_all(xyz, points):
    """-> new_xyz zeros [B,1,3], new_points [B,1,N,3+D] (pointnet2_utils.py:141-158)."""
    B, N, C = xyz.shape
    new_xyz = torch.zeros(B, 1, C, device=xyz.device, dtype=xyz.dtype)
    grouped_xyz = xyz.view(B, 1, N, C)
    if points is not None:
        return new_xyz, torch.cat([grouped_xyz, points.view(B, 1, N, -1)], dim=-1)
    return new_xyz, grouped_xyz


class PointNetSetAbstraction(nn.Module):
    """pointnet2_utils.py:161-202: sample npoint centroids, group nsample neighbours within radius,
    a shared Conv2d(1x1)+BatchNorm2d+ReLU stack, max over each group."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint = npoint
        self.radius = radius
        self.nsample = nsample
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last_channel = out_channel
        self.group_all = group_all

    def forward(self, xyz, points, start=None):
        """xyz [B,3,N], points [B,D,N] | None -> new_xyz [B,3,S], new_points [B,mlp[-1],S]."""
        xyz = xyz.permute(0, 2, 1).contiguous()
        if points is not None:
            points = points.permute(0, 2, 1).contiguous()
        B, N, _ = xyz.shape
        if self.group_all:
            new_xyz, new_points = sample_and_group_all(xyz, points)
            S, rows_per = 1, N
            x = new_points.reshape(B * N, -1)
        else:
            new_xyz, x, _, _ = _sample_and_group(self.npoint, self.radius, self.nsample, xyz, points, start)
            S, rows_per = self.npoint, self.nsample
        params = []
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            params += [conv.weight, conv.bias, bn.weight, bn.bias]
        spec = ChainSpec([K.ACT_ENC] * len(self.mlp_convs), rows_per, self.training, list(self.mlp_bns), pool=True)
        pooled, _ = PointChainFn.apply(spec, x, *params)
        return new_xyz.permute(0, 2, 1), pooled.view(B, S, -1).permute(0, 2, 1)


class PointNetSetAbstractionMsg(nn.Module):
    """pointnet2_utils.py:205-262: npoint centroids, and per scale (radius, nsample) a ball query, a
    grouping, a shared Conv2d(1x1)+BatchNorm2d+ReLU stack and a max over each group; the scales'
    outputs concatenated along channels."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint = npoint
        self.radius_list = radius_list
        self.nsample_list = nsample_list
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for mlp in mlp_list:
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last_channel = in_channel + 3
            for out_channel in mlp:
                convs.append(nn.Conv2d(last_channel, out_channel, 1))
                bns.append(nn.BatchNorm2d(out_channel))
                last_channel = out_channel
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward(self, xyz, points, start=None):
        """xyz [B,3,N], points [B,D,N] | None -> new_xyz [B,3,S], new_points [B,sum(mlp[-1]),S]."""
        xyz = xyz.permute(0, 2, 1).contiguous()
        D = 0
        if points is not None:
            points = points.permute(0, 2, 1).contiguous()
            D = points.shape[-1]
        B, S = xyz.shape[0], self.npoint
        fps_idx = G.fps(xyz, S, start)
        new_xyz = G.GroupFn.apply(None, None, xyz, fps_idx.view(B, S, 1)).view(B, S, 3)
        pooled = []
        for radius, nsample, convs, bns in zip(self.radius_list, self.nsample_list, self.conv_blocks, self.bn_blocks):
            idx = G.ball_query(radius, nsample, xyz, new_xyz)
            x = G.GroupFn.apply(xyz, new_xyz, points, idx)             # [B*S*nsample, 3 + D], xyz first
            params = []
            for j, (conv, bn) in enumerate(zip(convs, bns)):
                W = conv.weight
                if j == 0 and D:     # the reference cats [points, xyz - centre]: rotate the columns, not the matrix
                    W = W.view(W.shape[0], -1)
                    W = torch.cat([W[:, D:], W[:, :D]], dim=1)
                params += [W, conv.bias, bn.weight, bn.bias]
            spec = ChainSpec([K.ACT_ENC] * len(convs), nsample, self.training, list(bns), pool=True)
            out, _ = PointChainFn.apply(spec, x, *params)
            pooled.append(out.view(B, S, -1))
        return new_xyz.permute(0, 2, 1), torch.cat(pooled, dim=-1).permute(0, 2, 1)


class PointNetFeaturePropagation(nn.Module):
    """pointnet2_utils.py:265-315: the coarse features points2 (at xyz2) interpolated to the fine
    cloud xyz1 with inverse-distance weights over the three nearest coarse points, concatenated
    behind the skip features points1, then a shared Conv1d+BatchNorm1d+ReLU stack."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv1d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out_channel))
            last_channel = out_channel

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] | None, points2 [B,D2,S] -> [B,mlp[-1],N]."""
        xyz1 = xyz1.permute(0, 2, 1).contiguous()
        xyz2 = xyz2.permute(0, 2, 1).contiguous()
        points2 = points2.permute(0, 2, 1).contiguous()
        if points1 is not None:
            points1 = points1.permute(0, 2, 1).contiguous()
        B, N, _ = xyz1.shape
        if xyz2.shape[1] == 1:       # one coarse point: its features for every fine point (the reference's repeat)
            d2 = torch.zeros(B, N, 1, device=xyz1.device)
            idx = torch.zeros(B, N, 1, dtype=torch.int32, device=xyz1.device)
        else:
            d2, idx = I.three_nn(xyz1, xyz2)
        x = I.InterpFn.apply(points1, points2, idx, d2)
        params = []
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            params += [conv.weight, conv.bias, bn.weight, bn.bias]
        spec = ChainSpec([K.ACT_ENC] * len(self.mlp_convs), N, self.training, list(self.mlp_bns), pool=False, want_act=True)
        _, act = PointChainFn.apply(spec, x, *params)
        return act.view(B, N, -1).permute(0, 2, 1)
