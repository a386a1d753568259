"""CPU checks of the feature-propagation oracle chain: tests/fp_ref.py (the plain restatement of the
contracts of csrc/interp.hip and of the FP / MSG layers) against tests/golden/fp.npz (the
reference's pointnet2_utils.py, written by tests/golden/make_golden_fp.py), the constants of the
kernel bounds of tests/test_fp_gpu.py on the fp32 restatement, the argument validation of the new
entry points (which precedes any device work), and the state_dict layouts of the two layers and
the six pointnet2_* models."""
import os

import numpy as np
import pytest

import fp_ref as R
import group_ref as GR
from conftest import GOLDEN
from fp_ref import CASES, MSG, fp_ref_layer, msg_ref_layer, sd_of

MODELS = {"pointnet2_cls_ssg": (40, True), "pointnet2_cls_msg": (40, True), "pointnet2_part_seg_ssg": (50, True),
          "pointnet2_part_seg_msg": (50, True), "pointnet2_sem_seg": (13,), "pointnet2_sem_seg_msg": (13,)}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "fp.npz")))


def _close(got, want, what, rel=1e-11):
    assert got.shape == want.shape, what
    err = np.abs(got - want).max()
    assert err <= rel * max(1.0, np.abs(want).max()), f"{what}: {err:.3e}"


def _tol(r32, r64):
    return 3 * np.abs(r32["out"] - r64["out"]).max() + 1e-5 * np.abs(r64["out"]).max()


def test_golden_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "fp.npz")) < 512 * 1024


def test_fp_a_third_neighbour_is_clear_and_coarse_is_a_subset(gold):
    """(ii): every query's (d4 - d3) / d4 >= 1e-3, so fp32 and float64 pick the same three
    neighbours; the coarse cloud is a subset: d = 0 for S = 48 points of every cloud."""
    assert gold["fpa_xyz1"].shape == (2, 192, 3) and gold["fpa_xyz2"].shape == (2, 48, 3)
    assert R.neighbour_gap(gold["fpa_xyz1"], gold["fpa_xyz2"]) >= 1e-3
    d, _ = R.three_nn(gold["fpa_xyz1"], gold["fpa_xyz2"])
    assert ((d[..., 0] == 0).sum(-1) == 48).all()
    assert gold["fpb_xyz2"].shape[1] == 1 and "fpb_points1" not in gold


@pytest.mark.parametrize("tag", ["fpa", "fpb"])
def test_fp_layer_ref_equals_reference_and_decisions_are_clear(gold, tag):
    """(i) and (iii) for the feature-propagation cases."""
    import torch
    r64, r32 = fp_ref_layer(gold, tag, torch.float64), fp_ref_layer(gold, tag, torch.float32)
    for k in ("out", "gxyz1", "gxyz2", "gpoints2") + (("gpoints1",) if tag == "fpa" else ()):
        _close(r64[k], gold[f"{tag}_ref_{k}"], k)
    for k, v in r64["grads"].items():
        _close(v, gold[f"{tag}_grad_{k}"], k)
    for k, v in r64["running"].items():
        _close(v, gold[f"{tag}_after_{k}"], k)
    assert R.relu_margin(r64["pre"]) > 2 * _tol(r32, r64)


def test_msg_layer_ref_equals_reference_and_decisions_are_clear(gold):
    """(i) and (iii) for the multi-scale layer, on a grid cloud (coordinates k/8)."""
    import torch
    k8 = gold["msg_xyz"].astype(np.float64) * 8
    assert (k8 == np.round(k8)).all() and np.abs(k8).max() <= 8
    r64, r32 = msg_ref_layer(gold, torch.float64), msg_ref_layer(gold, torch.float32)
    for k in ("out", "new_xyz", "gxyz", "gpoints"):
        _close(r64[k], gold[f"msg_ref_{k}"], k)
    for k, v in r64["grads"].items():
        _close(v, gold[f"msg_grad_{k}"], k)
    for k, v in r64["running"].items():
        _close(v, gold[f"msg_after_{k}"], k)
    tol = _tol(r32, r64)
    margins = [GR.decision_margin(p) for p in r64["pre"]]
    assert min(m[0] for m in margins) > 2 * tol and min(m[1] for m in margins) > 2 * tol, (margins, tol)


# ---------------- the kernel bounds on the fp32 restatement ----------------

@pytest.mark.parametrize("B,N,S,D2,D1,coincident", CASES)
def test_fp32_restatement_meets_the_kernel_bounds(B, N, S, D2, D1, coincident):
    """The fp32 numpy restatement of the kernels against float64 under the bounds of
    tests/test_fp_gpu.py: forward 10 u sum|w f| (it needs 4.3 on these cases), grad_points2
    (n_e + 8) u sum|terms| (n_e + 1.5 at worst), grad_d2 (D2 + 16) u T_e (4.5 at worst) and finite.
    The constants are validated here, without a GPU; the figures are printed."""
    c = R.kernel_case(B, N, S, D2, D1, coincident)
    K = min(3, S)
    assert c["idx"].shape == (B, N, K)
    assert ((c["d2"][..., 0] == 0).sum(-1) >= (S - 1 if coincident else S)).all()       # the coarse cloud is a subset
    if coincident:
        assert (c["d2"][..., :2] == 0).all(-1).any()           # a fine point with two coincident neighbours
    out, w = R.interp_fwd32(c["points2"], c["idx"], c["d2"], c["points1"])
    R.check_fwd(out, c)
    if K == 1:
        assert (w == 1).all()
        want = np.repeat(c["points2"], N, axis=1).reshape(B * N, D2)
        assert (out[:, D1:].view(np.uint32) == want.view(np.uint32)).all()
    b = R.interp_bwd32(c["g"], c["points2"], c["idx"], c["d2"], D1)
    R.check_bwd(b["gp2"], b["gd2"], c)
    if K == 1:
        assert not b["gd2"].any()
    if (N, S) == (200, 3):
        assert R.interp_bwd64(c["g"], c["points2"], c["idx"], c["d2"], D1)["n2"].min() == 200


def test_naive_weight_gradient_misses_the_bound():
    """The form -r_k w_k sum_c g_c (f_kc - out_c) in fp32 misses (D2 + 16) u T_e by orders of
    magnitude where d_k = 0: the reason the contract spells out the other form."""
    c = R.kernel_case(2, 256, 64, 37, 0)
    w, r = R.weights32(c["d2"])
    f = R._gather(c["points2"], c["idx"])
    out, _ = R.interp_fwd32(c["points2"], c["idx"], c["d2"])
    g = c["g"].reshape(2, 256, 1, 37)
    naive = -(r * w) * (g * (f - out.reshape(2, 256, 1, 37))).sum(-1, dtype=np.float32)
    ref = R.interp_bwd64(c["g"], c["points2"], c["idx"], c["d2"], 0)
    ratio = (np.abs(naive - ref["gd2"]) / (R.U * ref["Te"])).max()
    assert ratio > 1e4 * (37 + R.C_GD2), ratio


# ---------------- argument validation, no GPU ----------------

def test_interp_abi_limits_without_gpu(built):
    from ured_hip import _lib, interp  # noqa: F401  (binds the entry points)
    one = 8    # any non-null value: validation never dereferences

    def fwd(B, N, S, K, D1, D2, p1=None, rest=None):
        _lib.call("ured_interp_fwd", rest, rest, rest, p1, B, N, S, K, D1, D2, rest, rest, None)

    def bwd(B, N, S, K, D1, D2, rest=None):
        _lib.call("ured_interp_bwd", rest, rest, rest, rest, rest, B, N, S, K, D1, D2, rest, rest, None)

    for who, fn in (("ured_interp_fwd", fwd), ("ured_interp_bwd", bwd)):
        with pytest.raises(_lib.UredError, match=who + r": K 0 outside \[1, 3\]"):
            fn(1, 8, 4, 0, 0, 2)
        with pytest.raises(_lib.UredError, match=who + r": K 4 outside \[1, 3\]"):
            fn(1, 8, 4, 4, 0, 2)
        with pytest.raises(_lib.UredError, match="N 0 and S 4 must be at least 1"):
            fn(1, 0, 4, 3, 0, 2)
        with pytest.raises(_lib.UredError, match="N 8 and S 0 must be at least 1"):
            fn(1, 8, 0, 3, 0, 2)
        with pytest.raises(_lib.UredError, match="D2 0 must be at least 1"):
            fn(1, 8, 4, 3, 0, 0)
        with pytest.raises(_lib.UredError, match="B 65536 exceeds 65535"):
            fn(65536, 8, 4, 3, 0, 2)
        with pytest.raises(_lib.UredError, match=r"B \* N \* \(D1 \+ D2\) = 2147483648 exceeds 2\^31 - 1"):
            fn(64, 1 << 15, 4, 3, 512, 512)
        with pytest.raises(_lib.UredError, match=r"B \* S \* D2 = 2147483648 exceeds 2\^31 - 1"):
            fn(64, 4, 1 << 15, 3, 0, 1024)
        with pytest.raises(_lib.UredError, match="negative size"):
            fn(-1, 8, 4, 3, 0, 2)
        with pytest.raises(_lib.UredError, match="null pointer"):
            fn(1, 8, 4, 3, 0, 2)
        fn(0, 8, 4, 3, 0, 2)                     # B = 0: a no-op
    with pytest.raises(_lib.UredError, match="points1 and D1 > 0 go together"):
        fwd(1, 8, 4, 3, 2, 2, rest=one)
    with pytest.raises(_lib.UredError, match="points1 and D1 > 0 go together"):
        fwd(1, 8, 4, 3, 0, 2, p1=one, rest=one)
    fwd(0, 8, 4, 3, 2, 2, p1=one)
    assert _lib.lib().ured_last_error() == b""


def test_python_argument_checks_without_gpu(built):
    import torch
    from ured_hip import interp
    x, p2 = torch.zeros(2, 8, 3), torch.zeros(2, 4, 5)
    idx, d2 = torch.zeros(2, 8, 3, dtype=torch.int32), torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        interp.three_nn(x, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        interp.InterpFn.apply(None, p2, idx, d2)
    from network.pointnet.pointnet2_utils import PointNetFeaturePropagation, PointNetSetAbstractionMsg
    with pytest.raises(RuntimeError, match="MI355X only"):
        PointNetFeaturePropagation(5, [4])(x.permute(0, 2, 1), x[:, :4].permute(0, 2, 1), None, p2.permute(0, 2, 1))
    with pytest.raises(RuntimeError, match="MI355X only"):
        PointNetSetAbstractionMsg(4, [0.1], [2], 0, [[4]])(x.permute(0, 2, 1), None)


# ---------------- state_dict layouts ----------------

def test_state_dict_keys_of_the_layers(gold, built):
    import torch
    from network.pointnet.pointnet2_utils import PointNetFeaturePropagation, PointNetSetAbstractionMsg
    T = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    fp = PointNetFeaturePropagation(6 + 10, [32, 16])
    fp.load_state_dict(T(sd_of(gold, "fpa")), strict=True)
    assert fp.mlp_convs[0].weight.shape == (32, 16, 1) and isinstance(fp.mlp_bns[1], torch.nn.BatchNorm1d)
    PointNetFeaturePropagation(12, [16]).load_state_dict(T(sd_of(gold, "fpb")), strict=True)
    msg = PointNetSetAbstractionMsg(MSG["npoint"], MSG["radius_list"], MSG["nsample_list"], 5, [[16, 32], [16, 24]])
    msg.load_state_dict(T(sd_of(gold, "msg")), strict=True)
    assert msg.conv_blocks[1][0].weight.shape == (16, 8, 1, 1) and isinstance(msg.bn_blocks[0][1], torch.nn.BatchNorm2d)
    assert "conv_blocks.1.1.weight" in msg.state_dict() and "bn_blocks.0.0.running_var" in msg.state_dict()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_state_dict_keys_and_shapes_of_the_models(gold, built, name):
    """A CPU construction (no forward): the keys, in order, and the shapes of the reference's model."""
    import importlib
    model = importlib.import_module("network.pointnet." + name).get_model(*MODELS[name])
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold[f"model_{name}_keys"]]
    for v, want in zip(sd.values(), gold[f"model_{name}_shapes"]):
        assert list(v.shape) == [int(s) for s in want if s >= 0]
    assert hasattr(importlib.import_module("network.pointnet." + name), "get_loss")
