"""Drop-in for the reference network/VN/vn_retrieval.py (vn_retrieval): the VN-DGCNN encoder of the
retrieval branch, vn_encoder without the per-point head; it returns the global feature alone. Same
constructor arguments, cfg keys and state_dict keys as the reference.
"""
import torch.nn as nn

from network.VN.vn_layers import *  # noqa: F401,F403  (the reference's import)
from network.VN.vn_dgcnn_util import get_graph_feature  # noqa: F401
from network.VN.vn_encoder import build_trunk, global_rows, trunk_rows


class vn_retrieval(nn.Module):
    def __init__(self, cfg, num_class=40, normal_channel=False):
        super(vn_retrieval, self).__init__()
        self.args = cfg
        self.n_knn = cfg['n_knn']
        build_trunk(self, cfg, per_point=False)

    def forward(self, x):
        return global_rows(self, trunk_rows(self, x))
