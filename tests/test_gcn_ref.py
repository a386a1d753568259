"""tests/gcn_ref.py pinned to tests/golden/gcn.npz (the reference's network/P_3DGC.py and
network/gc3d_encoder.py in float64): indices exactly, values and gradients to float64 round-off. Also
asserted here, for the reference alone: the conditions that make the GPU comparison of
tests/test_gcn_gpu.py meaningful (see tests/golden/make_golden_gcn.py), and the argument validation of
ured_hip.gcn and of the encoder, which runs before any device work and so needs no GPU."""
import os

import numpy as np
import pytest
import torch

import gcn_ref as R
from conftest import GOLDEN

RT = 1e-11          # float64 round-off, relative to the tensor's largest magnitude
MOD = dict(B=2, V=64, n=4, S=3, cin=4, cout=8)


@pytest.fixture(scope="module")
def gold():
    path = os.path.join(GOLDEN, "gcn.npz")
    assert os.path.getsize(path) < 512 * 1024
    return dict(np.load(path))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _close(got, want, what):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    assert err <= RT * max(want.abs().max().item(), 1.0), f"{what}: err {err:.3e}"


# ---------------- kernel-level cases: their conditions ----------------

@pytest.mark.parametrize("ci", range(len(R.KERNEL_CASES)))
@pytest.mark.parametrize("layer", [False, True])
def test_kernel_case_conditions(gold, ci, layer):
    case = R.KERNEL_CASES[ci]
    dirn, sdn, feat, idx, g = R.kernel_case(case, int(gold["kern_seeds"][ci, int(layer)]), layer)
    for t in (dirn, sdn):
        assert bool(((t * 8).round() == t * 8).all()) and t.abs().max() <= 1
    gap, _, mx, nzero, exact = R.winner_gaps(dirn, sdn, feat, idx, case[3])
    assert nzero > 0, "theta == 0 must occur"
    assert exact, "every product must be exact in fp32"
    assert gap > 1e-5 * mx
    B, V, n, S, C = case
    th = R._theta(dirn, sdn, S)[1]
    assert bool((th[:, 0] == 0).all())
    if V > 1:
        assert bool((th[:, 1, :, 0] <= 0).all()), "vertex 1, support 0: every theta <= 0"
    assert int((idx == 0).sum()) >= idx.numel() // 4, "index 0 is shared by many vertices"
    # the explicit backward equals autograd through the plain composition at the chosen slots
    out, slot = R.conv_fwd(dirn, sdn, feat, idx, S)
    gf, gs = R.conv_bwd(g, dirn, sdn, feat, idx, slot, S)
    sd = sdn.clone().requires_grad_(True)
    ft = None if feat is None else feat.clone().requires_grad_(True)
    prod = R._products(dirn, sd, ft, idx, S)[0]
    picked = torch.gather(prod, 2, slot.view(B, V, 1, S, C)).squeeze(2).sum(2)
    if ft is not None:
        picked = picked + ft.view(B, V, S + 1, C)[:, :, 0]
    _close(picked.reshape(B * V, C), out, "forward")
    # torch's relu has gradient 0 at theta == 0, as the contract's "iff theta > 0"
    picked.reshape(B * V, C).backward(g)
    _close(gs, sd.grad, "grad_sdn")
    if ft is not None:
        _close(gf, ft.grad, "grad_feat")


# ---------------- modules against the reference ----------------

def test_indices_vs_golden(gold):
    v = _t(gold["mod_vertices"])
    assert R.cloud_ok(v, MOD["n"]), "K-NN distances through rank n + 2 must be separated by more than 1e-6"
    idx = R.get_neighbor_index(v, MOD["n"])
    np.testing.assert_array_equal(idx.numpy(), gold["mod_idx"])
    vp = _t(gold["mod_pool_v"])
    ds = R.knn_index(v, vp, 1)[1]
    assert R.sorted_gaps_ok(ds, 2), "every nearest-vertex choice must lead the second by more than 1e-6"
    np.testing.assert_array_equal(R.get_nearest_index(v, vp).numpy(), gold["mod_nearest"])
    d = R.dirs(v, idx)
    _close(d.norm(dim=-1), torch.ones(2, 64, 4, dtype=torch.float64), "unit directions")


def test_conv_surface_vs_golden(gold):
    v, idx = _t(gold["mod_vertices"]), _t(gold["mod_idx"]).long()
    d = _t(gold["mod_surf.directions"]).requires_grad_(True)
    y = R.conv_surface(d, MOD["S"], idx, v)
    y.backward(_t(gold["mod_g"]))
    _close(y.detach(), gold["mod_surf_out"], "out")
    _close(d.grad, gold["mod_surf_gdir"], "grad directions")


def test_conv_layer_vs_golden(gold):
    v, idx = _t(gold["mod_vertices"]), _t(gold["mod_idx"]).long()
    w, b, d = (_t(gold["mod_layer." + k]).requires_grad_(True) for k in ("weights", "bias", "directions"))
    x = _t(gold["mod_fmap"]).requires_grad_(True)
    assert R.layer_case_ok(w.detach(), b.detach(), d.detach(), MOD["S"], idx, v, x.detach()), \
        "no theta within 2e-6 of 0 and no winner within 1e-5 * max of its runner-up"
    y = R.conv_layer(w, b, d, MOD["S"], idx, v, x)
    y.backward(_t(gold["mod_g"]))
    _close(y.detach(), gold["mod_layer_out"], "out")
    for got, key in ((w.grad, "gw"), (b.grad, "gb"), (d.grad, "gdir"), (x.grad, "gx")):
        _close(got, gold["mod_layer_" + key], key)


def test_pool_vs_golden(gold):
    v = _t(gold["mod_vertices"])
    x = _t(gold["mod_pmap"]).requires_grad_(True)
    sample = _t(gold["mod_pool_sample"]).long()
    torch.manual_seed(int(gold["mod_pool_seed"]))
    np.testing.assert_array_equal(torch.randperm(64)[:16].numpy(), sample.numpy())
    vp, fp = R.pool_layer(v, x, sample)
    fp.backward(_t(gold["mod_gp"]))
    _close(vp, gold["mod_pool_v"], "vertices_pool")
    _close(fp.detach(), gold["mod_pool_out"], "feature_map_pool")
    _close(x.grad, gold["mod_pool_gx"], "grad feature_map")
    # the explicit pool kernels' restatement agrees with it
    idx = R.get_neighbor_index(v, 4)
    out, slot = R.pool_fwd(x.detach().reshape(128, -1), idx, sample)
    assert bool((out.view(2, 16, -1) == fp.detach()).all())
    gx = R.pool_bwd(_t(gold["mod_gp"]).reshape(32, -1), idx, sample, slot, 64)
    _close(gx.view(2, 64, -1), gold["mod_pool_gx"], "pool_bwd")


@pytest.mark.parametrize("V", [128, 256])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_encoder_vs_golden(gold, V, mode):
    verts = _t(gold[f"enc{V}_vertices"])
    pseed, rseed, wseed = (int(s) for s in gold[f"enc{V}_seeds"])
    assert R.encoder_clouds_ok(verts, rseed), "K-NN / nearest-vertex gaps of the three levels"
    s0, s1 = R.encoder_samples(V, rseed)
    np.testing.assert_array_equal(s0.numpy(), gold[f"enc{V}_samples0"])
    np.testing.assert_array_equal(s1.numpy(), gold[f"enc{V}_samples1"])
    P = R.encoder_params(wseed)
    with torch.no_grad():
        fg, feat, stats = R.encoder(P, verts, mode == "train", (s0, s1))
    _close(fg, gold[f"enc{V}_{mode}_fglobal"], "f_global")
    _close(feat[:, :, ::16], gold[f"enc{V}_{mode}_feat_sub"], "feat")
    if mode == "train":
        for k, v in stats.items():
            _close(v, gold[f"enc{V}_train_{k}"], k)


# ---------------- argument validation (before any device work) ----------------

def test_validation_without_gpu(built):
    from ured_hip import gcn
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)    # noqa: E731
    z = torch.zeros
    with pytest.raises(ValueError, match="int32"):
        gcn.neighbor_dirs(z(2, 5, 3), torch.zeros(2, 5, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32"):
        gcn.neighbor_dirs(z(2, 5, 3, dtype=torch.float64), i32(2, 5, 4))
    with pytest.raises(ValueError, match=r"must be \[\*,\*,3\]"):
        gcn.neighbor_dirs(z(10, 3), i32(2, 5, 4))
    with pytest.raises(ValueError, match="does not match"):
        gcn.neighbor_dirs(z(2, 6, 3), i32(2, 5, 4))
    with pytest.raises(ValueError, match="requires grad"):
        gcn.neighbor_dirs(z(2, 5, 3, requires_grad=True), i32(2, 5, 4))
    with pytest.raises(ValueError, match=r"outside \[1, 255\]"):
        gcn.neighbor_dirs(z(1, 5, 3), i32(1, 5, gcn.GCN_NMAX + 1))
    conv = gcn.GcnConvFn.apply
    with pytest.raises(ValueError, match=r"support count 9 is outside \[1, 8\]"):
        conv(z(2, 5, 4, 3), z(3, 36), None, i32(2, 5, 4), gcn.GCN_SMAX + 1)
    with pytest.raises(ValueError, match="does not match"):
        conv(z(2, 5, 4, 3), z(3, 8), None, i32(2, 5, 3), 2)
    with pytest.raises(ValueError, match="not S \\* C"):
        conv(z(2, 5, 4, 3), z(3, 9), None, i32(2, 5, 4), 2)
    with pytest.raises(ValueError, match="feat must be"):
        conv(z(2, 5, 4, 3), z(3, 8), z(10, 8), i32(2, 5, 4), 2)
    with pytest.raises(ValueError, match="float32"):
        conv(z(2, 5, 4, 3), z(3, 8, dtype=torch.float64), None, i32(2, 5, 4), 2)
    with pytest.raises(ValueError, match=r"outside \[1, 255\]"):
        conv(z(1, 2, 256, 3), z(3, 8), None, i32(1, 2, 256), 2)
    pool = gcn.GcnPoolFn.apply
    with pytest.raises(ValueError, match=r"outside \[1, 255\]"):
        pool(z(10, 4), i32(2, 5, 300), i32(2))
    with pytest.raises(ValueError, match="sample must be int32"):
        pool(z(10, 4), i32(2, 5, 4), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="feat must be"):
        pool(z(11, 4), i32(2, 5, 4), i32(2))
    with pytest.raises(ValueError, match="weights must be"):
        gcn.GcnLinearFn.apply(z(10, 4), z(5, 8), z(8))
    # the C entry points refuse the same before any launch
    from ured_hip import _lib
    with pytest.raises(_lib.UredError, match="n 256 outside"):
        _lib.call("ured_gcn_dirs", None, None, 1, 5, 256, None, None)
    with pytest.raises(_lib.UredError, match="S 9 outside"):
        _lib.call("ured_gcn_conv_fwd", None, None, None, None, 1, 5, 4, 9, 8, None, None, None)
    with pytest.raises(_lib.UredError, match="workspace"):
        _lib.call("ured_gcn_conv_bwd", None, None, None, None, None, None, 1, 5, 4, 2, 8, None, None, None, 0, None)
    with pytest.raises(_lib.UredError, match="k 0 outside"):
        _lib.call("ured_gcn_pool_fwd", None, None, None, 1, 5, 0, 2, 8, None, None, None)
    assert _lib.query("ured_gcn_conv_bwd_parts", 2, 512) == gcn.bwd_parts(2, 512) == 64
    assert _lib.query("ured_gcn_conv_bwd_parts", 16, 2048) == gcn.bwd_parts(16, 2048) == gcn.GCN_BWD_PARTS
    assert _lib.query("ured_gcn_conv_bwd_parts", 1, 5) == gcn.bwd_parts(1, 5) == 1
    _lib.call("ured_gcn_dirs", None, None, 0, 5, 4, None, None)     # B = 0: a no-op that clears the message
    assert _lib.lib().ured_last_error() == b""


def test_encoder_refuses_small_clouds(built):
    from network.gc3d_encoder import GCN3D_ENCODER
    net = GCN3D_ENCODER()
    with pytest.raises(ValueError, match="at least 128"):
        net(torch.zeros(2, 64, 3))
    want = R.encoder_params(1)
    assert sorted(net.state_dict()) == sorted(want)
    assert all(tuple(net.state_dict()[k].shape) == tuple(want[k].shape) for k in want)
    net.load_state_dict(R.cast(want, torch.float32), strict=True)
