"""Drop-in for the reference network/VN/vn_dgcnn_util.py: knn and get_graph_feature with the
reference's signatures and layouts. The neighbour search runs on ured_hip.vn.knn_rows and follows
its order (direct squared distances, candidates ranked by (distance, index), the point itself
included), not the reference's expansion formula. get_graph_feature builds the reference's
[B, 2C, 3, N, k] tensor for callers that want it; the encoders never do, they hand the indices to the
fused layer (VNLinearLeakyReLU.forward_graph). get_graph_feature_cross is left out.
"""
import torch

from ured_hip import vn as V


def knn(x, k):
    """x [B, D, N] -> idx int64 [B, N, k]."""
    return V.knn_rows(x.detach().transpose(2, 1).contiguous().float(), k).long()


def get_graph_feature(x, k=20, idx=None, x_coord=None):
    """x [B, C, 3, N] -> [B, 2C, 3, N, k]: (x_j - x_i, x_i) over the k nearest neighbours j of i."""
    batch_size = x.size(0)
    num_points = x.size(3)
    x = x.view(batch_size, -1, num_points)
    if idx is None:
        if x_coord is None:  # dynamic knn graph
            idx = knn(x, k=k)
        else:  # fixed knn graph with input point coordinates
            idx = knn(x_coord, k=k)
    idx = idx.long()
    num_dims = x.size(1) // 3
    x = x.transpose(2, 1).contiguous()                       # [B, N, C*3]
    feature = x[torch.arange(batch_size, device=x.device).view(-1, 1, 1), idx]
    feature = feature.view(batch_size, num_points, k, num_dims, 3)
    x = x.view(batch_size, num_points, 1, num_dims, 3).expand(-1, -1, k, -1, -1)
    return torch.cat((feature - x, x), dim=3).permute(0, 3, 4, 1, 2).contiguous()
