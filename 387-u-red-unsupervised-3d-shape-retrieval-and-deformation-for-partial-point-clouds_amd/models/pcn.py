"""PCN (Density_aware_Chamfer_Distance/models/pcn.py:13-125) on the HIP Functions of ured_hip.pcn.

Same names, constructor arguments, parameter names and shapes as the reference (the layers are
nn.Conv1d / nn.Linear modules that only hold the parameters, so state_dicts interchange with
strict=True); `grid` is a plain attribute. Model.forward returns what the reference returns.
Unlike the reference, `alpha=None` in training and a `scale` that is not a power of two raise a
ValueError (the reference fails on a NoneType product and on a shape mismatch). Where the reference
keeps calc_emd's whole (emd, dist) tuple (training loss `emd`, whose .mean() then fails, and the
evaluation dict's 'emd'), this module takes the per-cloud emd [B].
"""
import torch
import torch.nn as nn

from chamfer3D.model_utils import calc_cd, calc_dcd, calc_emd, gen_grid_up
from ured_hip.pcn import MAX_SCALE, PcnDecoderFn, PcnEncoderFn


class PCN_encoder(nn.Module):
    def __init__(self, output_size=1024):
        super().__init__()
        self.conv1 = nn.Conv1d(3, 128, 1)
        self.conv2 = nn.Conv1d(128, 256, 1)
        self.conv3 = nn.Conv1d(512, 512, 1)
        self.conv4 = nn.Conv1d(512, output_size, 1)

    def forward(self, x, record=None):
        """x [B,3,N] -> global feature [B, output_size]."""
        return PcnEncoderFn.apply(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                  self.conv3.weight, self.conv3.bias, self.conv4.weight, self.conv4.bias, record)


class PCN_decoder(nn.Module):
    def __init__(self, num_coarse, num_fine, scale, cat_feature_num):
        super().__init__()
        scale = int(scale)
        if scale < 1 or scale & (scale - 1):
            raise ValueError(f"PCN_decoder: scale must be a power of two, got {scale}")
        if scale > MAX_SCALE:
            raise ValueError(f"PCN_decoder: scale {scale} exceeds {MAX_SCALE}")
        if num_fine != num_coarse * scale:
            raise ValueError(f"PCN_decoder: num_fine {num_fine} is not num_coarse {num_coarse} x scale {scale}")
        self.num_coarse = num_coarse
        self.num_fine = num_fine
        self.fc1 = nn.Linear(1024, 1024)
        self.fc2 = nn.Linear(1024, 1024)
        self.fc3 = nn.Linear(1024, num_coarse * 3)
        self.scale = scale
        self.grid = gen_grid_up(scale, 0.05)
        self.conv1 = nn.Conv1d(cat_feature_num, 512, 1)
        self.conv2 = nn.Conv1d(512, 512, 1)
        self.conv3 = nn.Conv1d(512, 3, 1)

    def forward(self, x, record=None):
        """x [B,1024] -> (coarse [B,3,num_coarse], fine [B,3,num_fine])."""
        if self.grid.device != x.device:
            self.grid = self.grid.to(x.device)
        return PcnDecoderFn.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.fc3.weight,
                                  self.fc3.bias, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                  self.conv3.weight, self.conv3.bias, self.grid, record)


class Model(nn.Module):
    def __init__(self, args, num_coarse=1024):
        super().__init__()
        self.num_coarse = num_coarse
        self.num_points = args.num_points
        self.train_loss = args.loss
        self.eval_emd = args.eval_emd
        self.scale = self.num_points // num_coarse
        self.cat_feature_num = 2 + 3 + 1024
        self.encoder = PCN_encoder()
        self.decoder = PCN_decoder(num_coarse, self.num_points, self.scale, self.cat_feature_num)
        self.loss_opts = args.loss_opts

    def forward(self, x, gt=None, is_training=True, alpha=None, test_emd=True):
        feat = self.encoder(x)
        out1, out2 = self.decoder(feat)
        out1 = out1.transpose(1, 2).contiguous()
        out2 = out2.transpose(1, 2).contiguous()
        if is_training:
            if alpha is None:
                raise ValueError("Model.forward: training needs alpha (the weight of the fine loss)")
            if self.train_loss == 'emd':
                loss1, _ = calc_cd(out1, gt)
                loss2, _ = calc_emd(out2, gt)
            elif self.train_loss == 'cd':
                loss1, _ = calc_cd(out1, gt)
                loss2, _ = calc_cd(out2, gt)
            elif self.train_loss == 'dcd':
                t_alpha, n_lambda = self.loss_opts["alpha"], self.loss_opts["lambda"]
                loss1, _, _ = calc_dcd(out1, gt, alpha=t_alpha, n_lambda=n_lambda)
                loss2, _, _ = calc_dcd(out2, gt, alpha=t_alpha, n_lambda=n_lambda)
            else:
                raise NotImplementedError(self.train_loss)
            total_train_loss = loss1.mean() + loss2.mean() * alpha
            return out2, loss2, total_train_loss, None
        if self.eval_emd and test_emd:
            emd, _ = calc_emd(out2, gt, eps=0.004, iterations=3000)
        else:
            emd = torch.ones(1, device=out2.device)
        _, cd_t, f1 = calc_cd(out2, gt, calc_f1=True)
        dcd, _, _ = calc_dcd(out2, gt)
        return {'out1': out1, 'out2': out2, 'emd': emd, 'dcd': dcd, 'cd_t': cd_t, 'f1': f1}
