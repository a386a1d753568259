"""Drop-in for the reference network/gc3d_encoder.py (GCN3D_ENCODER, after FS-Net): the 3D-GCN
encoder that returns the (global feature, per-point features) pair. Same constructor arguments,
module attributes and state_dict keys (conv_0..conv_4, bn1..bn3, conv1d_block.{0,1,3,4}), so a
reference checkpoint loads with strict=True.

The five graph convolutions and two poolings run on ured_hip.gcn (network/P_3DGC.py); each of the
three neighbourhoods' unit directions is computed once and shared by the layers on it; the three
nearest-vertex upsamplings are plain row gathers (ured_hip.group.GroupFn) into the point-major cat
that the fused Conv1d -> BatchNorm1d -> ReLU chain (ured_hip.mlp.PointChainFn) reads. bn1..bn3 are
the modules themselves on the [bs * vertice_num, C] view, which has the statistics of the
reference's (bs, C, vertice_num) call.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import network.P_3DGC as gcn3d
from ured_hip import kernels as K
from ured_hip.group import GroupFn
from ured_hip.mlp import ChainSpec, PointChainFn

MIN_VERTICES = 128      # below it the last level has vertice_num // 16 // 8 = 0 neighbours


class GCN3D_ENCODER(nn.Module):
    def __init__(self, gcn_n_num=10, gcn_sup_num=7):
        super(GCN3D_ENCODER, self).__init__()
        self.neighbor_num = gcn_n_num
        self.support_num = gcn_sup_num

        sup = self.support_num
        self.conv_0 = gcn3d.Conv_surface(kernel_num=128, support_num=sup)
        # (in, out) channels of conv_1..conv_4; a 4x pooling follows conv_1 and conv_3
        for i, (cin, cout) in enumerate([(128, 128), (128, 256), (256, 256), (256, 256)], start=1):
            setattr(self, f"conv_{i}", gcn3d.Conv_layer(cin, cout, support_num=sup))
        self.pool_1 = gcn3d.Pool_layer(pooling_rate=4, neighbor_num=4)
        self.pool_2 = gcn3d.Pool_layer(pooling_rate=4, neighbor_num=4)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(128), nn.BatchNorm1d(256), nn.BatchNorm1d(256)
        self.dim_fuse = 128 + 128 + 256 + 256 + 256          # fm_0..fm_4 side by side
        self.conv1d_block = nn.Sequential(nn.Conv1d(self.dim_fuse, 512, 1), nn.BatchNorm1d(512), nn.ReLU(inplace=True),
                                          nn.Conv1d(512, 256, 1), nn.BatchNorm1d(256), nn.ReLU(inplace=True))

    @staticmethod
    def _bn_relu(bn, fm):
        bs, v, c = fm.shape
        return F.relu(bn(fm.reshape(bs * v, c)), inplace=True).view(bs, v, c)

    @staticmethod
    def _upsample(fm, nearest):
        """fm (bs, v2, c), nearest long (bs, v1, 1) -> point-major [bs * v1, c]"""
        return GroupFn.apply(None, None, fm, nearest.to(torch.int32))

    def forward(self, vertices):
        """vertices (bs, vertice_num, 3) -> f_global (bs, 256), feat (bs, 256, vertice_num)"""
        bs, vertice_num, _ = vertices.size()
        if vertice_num < MIN_VERTICES:
            raise ValueError(f"GCN3D_ENCODER: {vertice_num} vertices, but at least {MIN_VERTICES} are needed: after "
                             "two 4x poolings the last level looks for vertice_num // 16 // 8 neighbours, which is 0 "
                             "below that (the reference fails there with a reshape error)")
        neighbor_index = gcn3d.get_neighbor_index(vertices, self.neighbor_num)
        dirn = gcn3d.get_neighbor_direction_norm(vertices, neighbor_index)
        fm_0 = F.relu(self.conv_0(neighbor_index, vertices, dirn), inplace=True)
        fm_1 = self._bn_relu(self.bn1, self.conv_1(neighbor_index, vertices, fm_0, dirn))
        v_pool_1, fm_pool_1 = self.pool_1(vertices, fm_1)

        neighbor_index = gcn3d.get_neighbor_index(v_pool_1, min(self.neighbor_num, v_pool_1.shape[1] // 8))
        dirn = gcn3d.get_neighbor_direction_norm(v_pool_1, neighbor_index)
        fm_2 = self._bn_relu(self.bn2, self.conv_2(neighbor_index, v_pool_1, fm_pool_1, dirn))
        fm_3 = self._bn_relu(self.bn3, self.conv_3(neighbor_index, v_pool_1, fm_2, dirn))
        v_pool_2, fm_pool_2 = self.pool_2(v_pool_1, fm_3)

        neighbor_index = gcn3d.get_neighbor_index(v_pool_2, min(self.neighbor_num, v_pool_2.shape[1] // 8))
        fm_4 = self.conv_4(neighbor_index, v_pool_2, fm_pool_2)
        f_global = fm_4.max(1)[0]

        nearest_pool_1 = gcn3d.get_nearest_index(vertices, v_pool_1)
        nearest_pool_2 = gcn3d.get_nearest_index(vertices, v_pool_2)
        m = bs * vertice_num
        x = torch.cat([fm_0.reshape(m, -1), fm_1.reshape(m, -1), self._upsample(fm_2, nearest_pool_1),
                       self._upsample(fm_3, nearest_pool_1), self._upsample(fm_4, nearest_pool_2)], dim=1)

        blk = self.conv1d_block
        params = [blk[0].weight, blk[0].bias, blk[1].weight, blk[1].bias,
                  blk[3].weight, blk[3].bias, blk[4].weight, blk[4].bias]
        spec = ChainSpec([K.ACT_ENC, K.ACT_ENC], vertice_num, self.training, [blk[1], blk[4]], pool=False, want_act=True)
        _, act = PointChainFn.apply(spec, x, *params)
        return f_global, act.view(bs, vertice_num, -1).permute(0, 2, 1)
