"""Drop-in for the reference network/P_3DGC.py (3D-GCN: Conv_surface, Conv_layer, Pool_layer and
their index helpers). Same names, signatures, tensor layouts, initialisation and state_dict keys
(`directions`, `weights`, `bias`), so a reference checkpoint loads with strict=True. The forward
and backward run on ured_hip.gcn: no [bs, vertice_num, neighbor_num, support_num * channel] tensor
is built. The neighbour search is ured_hip.nn.knn, which forms no [bs, v, v] matrix.

The layers take one argument more than the reference's: `neighbor_direction_norm`, the output of
get_neighbor_direction_norm for the same (vertices, neighbor_index), which layers that share a
neighbourhood compute once; left out, it is computed as in the reference. The vertex coordinates
are data here: the reference lets a gradient flow into them, which the encoder never asks for, and
vertices that require grad are refused with a ValueError in place of a silently missing gradient."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ured_hip import gcn as G
from ured_hip import nn as unn
from ured_hip.group import GroupFn


def get_neighbor_index(vertices, neighbor_num):
    """vertices (bs, vertice_num, 3) -> long (bs, vertice_num, neighbor_num): the neighbor_num + 1
    nearest vertices of every vertex without the first (the vertex itself, unless a duplicate with a
    lower index stands in front of it, as in the reference).

    The order is ured_hip.nn.knn's: the direct fp32 distance ((dx*dx) + (dy*dy)) + (dz*dz), sorted by
    (distance, index). The reference ranks |a|^2 + |b|^2 - 2ab from a bmm with topk; the two differ
    only where two candidates are closer in distance than fp32 rounding (on the CPU, uniform random
    clouds of 32-256 points gave no mismatch, 2 x 2048 points gave 3 mismatches in 40960 entries)."""
    v = vertices.detach()
    return unn.knn(v, v, int(neighbor_num) + 1)[1][:, :, 1:].long()


def get_nearest_index(target, source):
    """target (bs, v1, 3), source (bs, v2, 3) -> long (bs, v1, 1): the nearest source vertex of every
    target vertex (knn with K = 1; the lowest index wins a tie)."""
    return unn.knn(target.detach(), source.detach(), 1)[1].long()


def indexing_neighbor(tensor, index):
    """tensor (bs, v, dim), index long (bs, v', n) -> tensor[b, index] (bs, v', n, dim); differentiable
    in tensor (a deterministic scatter backward)."""
    bs, v, n = index.size()
    out = GroupFn.apply(None, None, tensor, index.to(torch.int32))
    return out.view(bs, v, n, tensor.shape[-1])


def get_neighbor_direction_norm(vertices, neighbor_index):
    """-> (bs, vertice_num, neighbor_num, 3): the unit vectors from every vertex to its neighbours
    (zero for a coincident neighbour). The coordinates are data: vertices that require grad are refused."""
    return G.neighbor_dirs(vertices, neighbor_index.to(torch.int32))


def _dirs(vertices, neighbor_index, neighbor_direction_norm):
    if neighbor_direction_norm is None:
        return get_neighbor_direction_norm(vertices, neighbor_index)
    return neighbor_direction_norm


class Conv_surface(nn.Module):
    """Extract structure feature from the surface, independent of the vertex coordinates
    (P_3DGC.py:72-112)."""

    def __init__(self, kernel_num, support_num):
        super().__init__()
        self.kernel_num = kernel_num
        self.support_num = support_num
        self.relu = nn.ReLU(inplace=True)
        self.directions = nn.Parameter(torch.FloatTensor(3, support_num * kernel_num))
        self.initialize()

    def initialize(self):
        stdv = 1. / math.sqrt(self.support_num * self.kernel_num)
        self.directions.data.uniform_(-stdv, stdv)

    def forward(self, neighbor_index, vertices, neighbor_direction_norm=None):
        """-> (bs, vertice_num, kernel_num)"""
        bs, vertice_num, _ = neighbor_index.size()
        dirn = _dirs(vertices, neighbor_index, neighbor_direction_norm)
        sdn = F.normalize(self.directions, dim=0)
        out, _ = G.GcnConvFn.apply(dirn, sdn, None, neighbor_index.to(torch.int32), self.support_num)
        return out.view(bs, vertice_num, self.kernel_num)


class Conv_layer(nn.Module):
    """P_3DGC.py:115-163: feature_map @ weights + bias on the MFMA GEMM, then the fused
    direction-weighted max over the neighbours and sum over the supports."""

    def __init__(self, in_channel, out_channel, support_num):
        super().__init__()
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.support_num = support_num
        self.relu = nn.ReLU(inplace=True)
        self.weights = nn.Parameter(torch.FloatTensor(in_channel, (support_num + 1) * out_channel))
        self.bias = nn.Parameter(torch.FloatTensor((support_num + 1) * out_channel))
        self.directions = nn.Parameter(torch.FloatTensor(3, support_num * out_channel))
        self.initialize()

    def initialize(self):
        stdv = 1. / math.sqrt(self.out_channel * (self.support_num + 1))
        self.weights.data.uniform_(-stdv, stdv)
        self.bias.data.uniform_(-stdv, stdv)
        self.directions.data.uniform_(-stdv, stdv)

    def forward(self, neighbor_index, vertices, feature_map, neighbor_direction_norm=None):
        """feature_map (bs, vertice_num, in_channel) -> (bs, vertice_num, out_channel)"""
        bs, vertice_num, _ = neighbor_index.size()
        dirn = _dirs(vertices, neighbor_index, neighbor_direction_norm)
        sdn = F.normalize(self.directions, dim=0)
        feature_out = G.GcnLinearFn.apply(feature_map.reshape(bs * vertice_num, self.in_channel), self.weights,
                                          self.bias)
        out, _ = G.GcnConvFn.apply(dirn, sdn, feature_out, neighbor_index.to(torch.int32), self.support_num)
        return out.view(bs, vertice_num, self.out_channel)


class Pool_layer(nn.Module):
    """P_3DGC.py:166-190. The sample is torch.randperm(vertice_num)[:pool_num] on the CPU generator,
    as in the reference, so a seeded run keeps the reference's vertices; only those are pooled."""

    def __init__(self, pooling_rate: int = 4, neighbor_num: int = 4):
        super().__init__()
        self.pooling_rate = pooling_rate
        self.neighbor_num = neighbor_num

    def forward(self, vertices, feature_map):
        """-> vertices_pool (bs, pool_num, 3), feature_map_pool (bs, pool_num, channel_num)"""
        bs, vertice_num, _ = vertices.size()
        v = vertices.detach()
        neighbor_index = unn.knn(v, v, self.neighbor_num + 1)[1][:, :, 1:]
        pool_num = int(vertice_num / self.pooling_rate)
        sample_idx = torch.randperm(vertice_num)[:pool_num].to(vertices.device)
        vertices_pool = vertices[:, sample_idx, :]
        pooled, _ = G.GcnPoolFn.apply(feature_map.reshape(bs * vertice_num, -1), neighbor_index,
                                      sample_idx.to(torch.int32))
        return vertices_pool, pooled.view(bs, pool_num, feature_map.shape[-1])
