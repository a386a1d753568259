"""The six pointnet2_* models on the GPU (network/pointnet/pointnet2_*.py): wiring, not parity. Layer
parity is the numeric claim (tests/test_group_gpu.py, tests/test_fp_gpu.py); a six-layer model has
too many ReLU and max-pool decisions to keep clear of rounding.

Each model runs on B = 2, N = 256 in training mode after torch.manual_seed(0) (the clouds are
smaller than some npoint: farthest-point sampling allows that): output shapes; exp(log_softmax)
rows sum to 1 within 1e-5 (a softmax over at most 50 classes in fp32: a sum of at most 50 terms in
[0,1], each within a few 2^-24 relative, is within 50 * 4 * 2^-24 < 1.2e-5 of 1, and far closer in
practice); every parameter gets a finite gradient; a second run after the same seed is bitwise equal
in outputs and gradients (sampling starts, dropout masks and every kernel of this package are
deterministic; the heads' torch Conv1d asks the vendor library for its deterministic algorithms
through torch.backends.cudnn.deterministic, as a user who wants reproducible runs would: without it
the weight gradient of the last Conv1d differed between two runs, everything else being equal)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, N = 2, 256
# name -> (constructor arguments, input channels, needs a one-hot label, classes, per-point output, feature shape)
MODELS = {
    "pointnet2_cls_ssg": ((40, True), 6, False, 40, False, (B, 1024, 1)),
    "pointnet2_cls_msg": ((40, True), 6, False, 40, False, (B, 1024, 1)),
    "pointnet2_part_seg_ssg": ((50, True), 6, True, 50, True, (B, 1024, 1)),
    "pointnet2_part_seg_msg": ((50, True), 6, True, 50, True, (B, 1024, 1)),
    "pointnet2_sem_seg": ((13,), 9, False, 13, True, (B, 512, 16)),
    "pointnet2_sem_seg_msg": ((13,), 9, False, 13, True, (B, 1024, 16)),
}


def _run(name, dev):
    args, cin, label, _, _, _ = MODELS[name]
    rng = np.random.default_rng(11)
    x = torch.from_numpy((rng.random((B, cin, N), dtype=np.float32) * 2 - 1).astype(np.float32)).to(dev)
    torch.manual_seed(0)
    model = importlib.import_module("network.pointnet." + name).get_model(*args).to(dev).train()
    ins = [x]
    if label:
        ins.append(torch.nn.functional.one_hot(torch.tensor([3, 11]), 16).float().to(dev))
    logp, feat = model(*ins)
    w = torch.from_numpy(rng.standard_normal(tuple(logp.shape)).astype(np.float32)).to(dev)
    ((logp * w).sum() + feat.sum()).backward()
    return model, logp, feat


@pytest.fixture(autouse=True)
def _deterministic_torch_convs(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_trains_one_step_deterministically(dev, built, name):
    _, _, _, classes, per_point, feat_shape = MODELS[name]
    model, logp, feat = _run(name, dev)
    assert tuple(logp.shape) == ((B, N, classes) if per_point else (B, classes))
    assert tuple(feat.shape) == feat_shape
    rows = logp.detach().exp().sum(-1)
    assert torch.isfinite(logp).all() and (rows - 1).abs().max().item() <= 1e-5
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    model2, logp2, feat2 = _run(name, dev)
    assert torch.equal(logp, logp2) and torch.equal(feat, feat2)
    for (k, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
