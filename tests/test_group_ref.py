"""CPU checks of the set-abstraction oracle chain: tests/group_ref.py (the plain restatement of the
contracts of csrc/group.hip) against tests/golden/group.npz (the reference's pointnet2_utils.py on
grid clouds, written by tests/golden/make_golden_group.py), and the argument validation of the new
entry points, which precedes any device work."""
import os

import numpy as np
import pytest

import group_ref as R
from conftest import GOLDEN

SA = dict(npoint=32, radius=0.25, nsample=16)
BALLS = [(0.25, 16), (0.5, 32), (0.125, 8)]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "group.npz")))


def test_golden_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "group.npz")) < 512 * 1024


@pytest.mark.parametrize("case,shape,npoint", [("a", (3, 64), 16), ("b", (2, 1000), 128), ("c", (2, 2048), 512),
                                               ("d", (2, 300), 300)])
def test_fps_ref_equals_reference(gold, case, shape, npoint):
    xyz, start, want = gold[f"fps_{case}_xyz"], gold[f"fps_{case}_start"], gold[f"fps_{case}_idx"]
    assert xyz.shape == shape + (3,) and want.shape == (shape[0], npoint)
    np.testing.assert_array_equal(R.fps(xyz, start, npoint), want)
    if case == "d":      # every point twice: the second half of the samples are all ties at distance 0
        assert all(len({tuple(p) for p in c}) <= 150 for c in xyz)


def test_golden_clouds_are_grid_points(gold):
    for case, g in (("a", 8), ("b", 64), ("c", 16), ("d", 8)):
        k = gold[f"fps_{case}_xyz"].astype(np.float64) * g
        assert (k == np.round(k)).all() and np.abs(k).max() <= g
    k = gold["sa_xyz"].astype(np.float64) * 8
    assert (k == np.round(k)).all() and np.abs(k).max() <= 8


@pytest.mark.parametrize("radius,nsample", BALLS)
def test_ball_query_ref_equals_reference(gold, radius, nsample):
    xyz, new_xyz, want = gold["fps_c_xyz"], gold["ball_new_xyz"], gold[f"ball_{radius}_{nsample}"]
    np.testing.assert_array_equal(R.ball_query(xyz, new_xyz, R.radius2(radius), nsample), want)


def test_ball_query_golden_covers_the_rules(gold):
    xyz, new_xyz = gold["fps_c_xyz"], gold["ball_new_xyz"]
    d = R.sqd(xyz[:, None, :, :], new_xyz[:, :, None, :])
    padded = full = boundary = 0
    for radius, nsample in BALLS:
        hits = (~(d > R.radius2(radius))).sum(-1)
        padded += int((hits < nsample).sum())
        full += int((hits >= nsample).sum())
        listed = np.take_along_axis(d, gold[f"ball_{radius}_{nsample}"].astype(np.int64), axis=-1)
        boundary += int((listed == R.radius2(radius)).sum())
    assert padded > 0 and full > 0 and boundary > 0


def test_ball_query_ref_rules():
    xyz = np.array([[[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 0.5, 0]]], np.float32)
    q = np.array([[[0, 0, 0], [5, 5, 5]]], np.float32)
    got = R.ball_query(xyz, q, np.float32(0.25), 3)
    np.testing.assert_array_equal(got[0, 0], [0, 2, 3])          # 0.25 is on the surface: included
    np.testing.assert_array_equal(got[0, 1], [4, 4, 4])          # no hit: N
    np.testing.assert_array_equal(R.ball_query(xyz, q, np.float32(0.0), 2)[0, 0], [0, 0])   # padded with the first


def test_group_ref_equals_reference(gold):
    rows = R.group_fwd(gold["sa_xyz"], gold["sg_new_xyz"], gold["sa_points"], gold["sg_idx"])
    np.testing.assert_array_equal(rows, gold["sg_new_points"].reshape(rows.shape))
    np.testing.assert_array_equal(R.fps(gold["sa_xyz"], gold["sa_start"], SA["npoint"]), gold["sg_fps_idx"])
    gx = R.group_fwd(None, None, gold["sa_xyz"], gold["sg_idx"])
    np.testing.assert_array_equal(gx, gold["sg_grouped_xyz"].reshape(gx.shape))


def test_group_ref_sentinel_and_bwd():
    rng = np.random.default_rng(0)
    xyz, pts = rng.standard_normal((1, 5, 3)).astype(np.float32), rng.standard_normal((1, 5, 2)).astype(np.float32)
    new = rng.standard_normal((1, 2, 3)).astype(np.float32)
    idx = np.array([[[0, 5, 0], [4, 4, 5]]], np.int32)
    rows = R.group_fwd(xyz, new, pts, idx)
    assert (rows[[1, 5]] == 0).all() and (rows[0] == np.concatenate([xyz[0, 0] - new[0, 0], pts[0, 0]])).all()
    g = rng.standard_normal(rows.shape).astype(np.float32)
    r = R.group_bwd(g, idx, 5, 3)
    np.testing.assert_array_equal(r["n"][0], [2, 0, 0, 0, 2])
    np.testing.assert_allclose(r["gx"][0, 0], g[0, :3].astype(np.float64) + g[2, :3], rtol=0, atol=0)
    np.testing.assert_allclose(r["gn"][0, 1], -(g[3, :3].astype(np.float64) + g[4, :3]), rtol=0, atol=0)
    np.testing.assert_allclose(r["gp"][0, 4], g[3, 3:].astype(np.float64) + g[4, 3:], rtol=0, atol=0)
    assert (r["gx"][0, 1:4] == 0).all()


def _sd(gold):
    return {k[len("sa_sd_"):]: v for k, v in gold.items() if k.startswith("sa_sd_")}


def _layer(gold, dtype, **kw):
    x = np.ascontiguousarray(gold["sa_xyz"].transpose(0, 2, 1))
    p = np.ascontiguousarray(gold["sa_points"].transpose(0, 2, 1))
    return R.sa_layer(_sd(gold), x, p, gold["sa_start"], SA["npoint"], SA["radius"], SA["nsample"], False, dtype,
                      gold["sa_g_out"], gold["sa_g_xyz"], **kw)


def test_sa_layer_ref_equals_reference_and_decisions_are_clear(gold):
    import torch
    r64, r32 = _layer(gold, torch.float64), _layer(gold, torch.float32)
    for k in ("out", "new_xyz", "gxyz", "gpoints"):
        want = gold[f"sa_ref_{k}"]
        assert np.abs(r64[k] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), k
    for k, v in r64["grads"].items():
        want = gold[f"sa_grad_{k}"]
        assert v.shape == want.shape and np.abs(v - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), k
    for k, v in r64["running"].items():
        assert np.abs(v - gold[f"sa_after_{k}"]).max() <= 1e-12, k
    # the precondition of the GPU test: no ReLU or max-pool decision within twice the forward tolerance
    tol = 3 * np.abs(r32["out"] - r64["out"]).max() + 1e-5 * np.abs(r64["out"]).max()
    relu_m, gap = R.decision_margin(r64["pre"])
    assert relu_m > 2 * tol and gap > 2 * tol, (relu_m, gap, tol)


def test_state_dict_keys_of_the_layer(gold, built):
    import torch
    from network.pointnet.pointnet2_utils import PointNetSetAbstraction
    layer = PointNetSetAbstraction(SA["npoint"], SA["radius"], SA["nsample"], 3 + 5, [16, 32], False)
    sd = {k: torch.from_numpy(v) for k, v in _sd(gold).items()}
    layer.load_state_dict(sd, strict=True)
    assert layer.mlp_convs[0].weight.shape == (16, 8, 1, 1) and isinstance(layer.mlp_bns[1], torch.nn.BatchNorm2d)


def test_group_abi_limits_without_gpu(built):
    from ured_hip import _lib, group  # noqa: F401  (binds the entry points)
    fps = lambda B, N, npoint: _lib.call("ured_fps", None, None, B, N, npoint, None, None)
    with pytest.raises(_lib.UredError, match=r"N 0 outside \[1, 16384\]"):
        fps(1, 0, 4)
    with pytest.raises(_lib.UredError, match=r"N 16385 outside \[1, 16384\]"):
        fps(1, 16385, 4)
    with pytest.raises(_lib.UredError, match="npoint 0 must be at least 1"):
        fps(1, 8, 0)
    with pytest.raises(_lib.UredError, match="B 65536 exceeds 65535"):
        fps(65536, 8, 2)
    with pytest.raises(_lib.UredError, match="null pointer"):
        fps(2, 8, 2)
    fps(0, 8, 2)
    bq = lambda B, N, S, r2, ns: _lib.call("ured_ball_query", None, None, B, N, S, r2, ns, None, None)
    with pytest.raises(_lib.UredError, match="N 0 and K 4 must be at least 1"):
        bq(1, 0, 4, 0.1, 4)
    with pytest.raises(_lib.UredError, match="N 8 and K 0 must be at least 1"):
        bq(1, 8, 4, 0.1, 0)
    with pytest.raises(_lib.UredError, match="is negative"):
        bq(1, 8, 4, -1.0, 4)
    with pytest.raises(_lib.UredError, match="exceeds 2\\^31 - 1"):
        bq(64, 4096, 4096, 0.1, 4096)
    with pytest.raises(_lib.UredError, match="null pointer"):
        bq(1, 8, 4, 0.1, 4)
    bq(1, 8, 0, 0.1, 4)
    gf = lambda B, N, S, K, D, xyz=None, new=None, pts=None: _lib.call("ured_group_fwd", xyz, new, pts, None, B, N, S, K, D,
                                                                      None, None)
    one = 8    # any non-null value: validation never dereferences
    with pytest.raises(_lib.UredError, match="xyz and new_xyz go together"):
        gf(1, 8, 4, 2, 0, xyz=one)
    with pytest.raises(_lib.UredError, match="points and D > 0 go together"):
        gf(1, 8, 4, 2, 3, xyz=one, new=one)
    with pytest.raises(_lib.UredError, match="nothing to gather"):
        gf(1, 8, 4, 2, 0)
    with pytest.raises(_lib.UredError, match="negative size"):
        gf(1, 8, -4, 2, 0, xyz=one, new=one)
    with pytest.raises(_lib.UredError, match="null pointer"):
        gf(1, 8, 4, 2, 0, xyz=one, new=one)
    gb = lambda B, N, S, K, D, gx=None, gn=None, gp=None: _lib.call("ured_group_bwd", None, None, B, N, S, K, D, gx, gn, gp,
                                                                   None)
    with pytest.raises(_lib.UredError, match="grad_xyz and grad_new_xyz go together"):
        gb(1, 8, 4, 2, 0, gx=one)
    with pytest.raises(_lib.UredError, match="grad_points and D > 0 go together"):
        gb(1, 8, 4, 2, 0, gx=one, gn=one, gp=one)
    with pytest.raises(_lib.UredError, match="null pointer"):
        gb(1, 8, 4, 2, 0, gx=one, gn=one)
    gb(0, 8, 4, 2, 0, gx=one, gn=one)
    assert _lib.lib().ured_last_error() == b""


def test_python_argument_checks_without_gpu(built):
    import torch
    from ured_hip import group
    x = torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        group.fps(x, 4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        group.ball_query(0.1, 4, x, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        group.GroupFn.apply(x, x, None, torch.zeros(2, 8, 2, dtype=torch.int32))
