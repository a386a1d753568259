"""PointNet++ part segmentation, single-scale grouping: the reference's network/pointnet/
pointnet2_part_seg_ssg.py (constructor arguments, forward signature, layer hyper-parameters,
attribute names and so state_dict keys, outputs) on the HIP set-abstraction and feature-propagation
layers of pointnet2_utils. The head (Conv1d / BatchNorm1d / Dropout / log_softmax) is plain torch."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from network.pointnet.pointnet2_utils import PointNetFeaturePropagation, PointNetSetAbstraction


class get_model(nn.Module):
    def __init__(self, num_classes, normal_channel=False):
        super().__init__()
        extra = 3 if normal_channel else 0
        self.normal_channel = normal_channel
        self.sa1 = PointNetSetAbstraction(512, 0.2, 32, 6 + extra, [64, 64, 128], False)
        self.sa2 = PointNetSetAbstraction(128, 0.4, 64, 128 + 3, [128, 128, 256], False)
        self.sa3 = PointNetSetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True)
        self.fp3 = PointNetFeaturePropagation(1280, [256, 256])
        self.fp2 = PointNetFeaturePropagation(384, [256, 128])
        self.fp1 = PointNetFeaturePropagation(128 + 16 + 6 + extra, [128, 128, 128])
        self.conv1 = nn.Conv1d(128, 128, 1)
        self.bn1 = nn.BatchNorm1d(128)
        self.drop1 = nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_classes, 1)

    def forward(self, xyz, cls_label):
        """xyz [B, 3 | 6, N], cls_label one-hot [B, 16] (any shape with B * 16 elements) ->
        log-probabilities [B, N, num_classes], the global feature [B, 1024, 1]."""
        B, _, N = xyz.shape
        l0_points = xyz
        l0_xyz = xyz[:, :3, :] if self.normal_channel else xyz
        l1_xyz, l1_points = self.sa1(l0_xyz, l0_points)
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points)
        l3_xyz, l3_points = self.sa3(l2_xyz, l2_points)
        l2_points = self.fp3(l2_xyz, l3_xyz, l2_points, l3_points)
        l1_points = self.fp2(l1_xyz, l2_xyz, l1_points, l2_points)
        one_hot = cls_label.view(B, 16, 1).repeat(1, 1, N)
        l0_points = self.fp1(l0_xyz, l1_xyz, torch.cat([one_hot, l0_xyz, l0_points], 1), l1_points)
        x = self.drop1(F.relu(self.bn1(self.conv1(l0_points))))
        x = F.log_softmax(self.conv2(x), dim=1)
        return x.permute(0, 2, 1), l3_points


class get_loss(nn.Module):
    def forward(self, pred, target, trans_feat):
        return F.nll_loss(pred, target)
