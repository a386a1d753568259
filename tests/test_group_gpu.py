"""Set abstraction on the GPU (csrc/group.hip, ured_hip/group.py, network/pointnet/
pointnet2_utils.py) against tests/group_ref.py and tests/golden/group.npz.

Indices (farthest-point sampling, ball query) and the grouping forward are compared bit for bit.
On the golden grid clouds that also pins them to the reference; on other inputs the GPU is compared
with group_ref only (the reference's |a|^2 + |b|^2 - 2ab rounds differently there).

Grouping backward: every output element e against the float64 sum of its terms,
|err(e)| <= (n_e + 1) * 2^-24 * sum|terms(e)|, n_e the element's number of contributions: the bound
of a sequential fp32 sum of n_e terms (n_e - 1 additions, each within 2^-24 relative of a partial
sum that is at most sum|terms| (1 + 2^-24)^n_e), plus the final rounding of the float64 reference.

Layer: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|, f = 1e-5 forward, 2e-5
gradients (the idiom of tests/test_chain_gpu.py), ref64 the golden (the reference's own layer in
float64), ref32 group_ref.sa_layer in float32 on the CPU; a conv bias in front of training-mode BN
has a zero true gradient and is bounded as there: max|g| <= 3 * max|g_ref32| + 1e-5 * max|dW_ref64|.
tests/test_group_ref.py asserts that no ReLU / max-pool decision of the golden layer lies within
twice the forward tolerance, so a flipped decision cannot pass for rounding or hide an error.
Nothing is derived from the GPU's output.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import group_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SA = dict(npoint=32, radius=0.25, nsample=16)
F_FWD, F_GRAD = 1e-5, 2e-5
U = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "group.npz")))


@pytest.fixture(scope="module")
def G(dev):
    from ured_hip import group
    return group


@pytest.fixture(autouse=True)
def _group_debug_word():
    """The debug build's bounds word of group.hip (file id 12), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_group"):
        return
    fn = mod._lib.ured_dbg_group
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): group.hip:{v & 0xFFFFFFFF}"


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _grid(rng, B, N, g):
    return (rng.integers(-g, g + 1, size=(B, N, 3)).astype(np.float32) / np.float32(g)).astype(np.float32)


# ---------------- farthest-point sampling ----------------

@pytest.mark.parametrize("kind", ["uniform", "grid"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 1025, 2048])
def test_fps_vs_ref(G, dev, N, kind):
    """B = 3 with start 0, N - 1 and one in between; npoint 1, 16, N and N + 5 (the longer runs are
    prefixes of one another, so the restatement runs once). The grid clouds (17 values per axis, and
    every point of the second half a copy) are full of ties and duplicates."""
    rng = np.random.default_rng(N * 2 + (kind == "grid"))
    if kind == "grid":
        xyz = _grid(rng, 3, N, 8)
        xyz[:, N // 2:] = xyz[:, :N - N // 2]
    else:
        xyz = rng.random((3, N, 3), dtype=np.float32) * 2 - 1
    start = np.array([0, N - 1, N // 3], np.int32)
    want = R.fps(xyz, start, max(16, N + 5))
    x, s = _t(xyz, dev), _t(start, dev)
    for npoint in (1, 16, N, N + 5):
        got = G.fps(x, npoint, s)
        assert got.dtype == torch.int32 and tuple(got.shape) == (3, npoint)
        np.testing.assert_array_equal(got.cpu().numpy(), want[:, :npoint], err_msg=f"npoint {npoint}")


@pytest.mark.parametrize("case,npoint", [("a", 16), ("b", 128), ("c", 512), ("d", 300)])
def test_fps_vs_golden(G, dev, gold, case, npoint):
    got = G.fps(_t(gold[f"fps_{case}_xyz"], dev), npoint, _t(gold[f"fps_{case}_start"], dev))
    np.testing.assert_array_equal(got.cpu().numpy(), gold[f"fps_{case}_idx"])


def test_fps_nmax_and_start_rules(G, dev):
    rng = np.random.default_rng(5)
    N = G.FPS_NMAX
    xyz = rng.random((1, N, 3), dtype=np.float32)
    start = np.array([N - 1], np.int32)
    got = G.fps(_t(xyz, dev), 8, _t(start, dev))
    np.testing.assert_array_equal(got.cpu().numpy(), R.fps(xyz, start, 8))
    # a start outside the cloud is clamped on the device; int64 starts are accepted
    x = _t(xyz[:, :100], dev)
    for s, c in ((-7, 0), (10 ** 6, 99)):
        got = G.fps(x, 5, torch.tensor([s], device=dev, dtype=torch.int64))
        np.testing.assert_array_equal(got.cpu().numpy(), R.fps(xyz[:, :100], [c], 5))
    # start=None draws on the device: a valid sample that follows the recurrence from its own start
    got = G.fps(x, 6).cpu().numpy()
    np.testing.assert_array_equal(got, R.fps(xyz[:, :100], got[:, 0], 6))


# ---------------- ball query ----------------

@pytest.mark.parametrize("radius,nsample", [(0.25, 16), (0.5, 32), (0.125, 8)])
def test_ball_query_vs_golden(G, dev, gold, radius, nsample):
    got = G.ball_query(radius, nsample, _t(gold["fps_c_xyz"], dev), _t(gold["ball_new_xyz"], dev))
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), gold[f"ball_{radius}_{nsample}"])


@pytest.mark.parametrize("nsample", [1, 8, 32, 64, 100])
@pytest.mark.parametrize("N,S,members", [(70, 1, True), (300, 65, False), (1000, 512, True), (65, 65, False)])
def test_ball_query_vs_ref(G, dev, N, S, members, nsample):
    """Member queries (the first S points, S <= N, or a cycle of them) and free queries in a larger
    box, so that some rows are empty (all N); nsample 100 exceeds N = 70 and N = 65."""
    rng = np.random.default_rng(N + S + nsample)
    xyz = rng.random((2, N, 3), dtype=np.float32)
    q = xyz[:, np.arange(S) % N] if members else (rng.random((2, S, 3), dtype=np.float32) * 2.0 - 0.5)
    radius = 0.2
    want = R.ball_query(xyz, q, R.radius2(radius), nsample)
    if not members:
        assert (want == N).all(-1).any() and (want != N).any()
    got = G.ball_query(radius, nsample, _t(xyz, dev), _t(q, dev))
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_ball_query_radius_zero(G, dev):
    rng = np.random.default_rng(9)
    xyz = _grid(rng, 2, 200, 2)                       # 125 cells for 200 points: duplicates
    q = np.concatenate([xyz[:, :40], rng.random((2, 3, 3), dtype=np.float32) + 2], 1)
    want = R.ball_query(xyz, q, np.float32(0), 4)
    assert (want[:, 40:] == 200).all() and (want[:, :40] < 200).all()
    got = G.ball_query(0.0, 4, _t(xyz, dev), _t(q, dev))
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---------------- grouping ----------------

def _group_case(D, seed, B=2, N=100, S=9, K=7, degenerate=False):
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((B, N, 3)).astype(np.float32)
    new = rng.standard_normal((B, S, 3)).astype(np.float32)
    pts = rng.standard_normal((B, N, D)).astype(np.float32) if D else None
    if degenerate:
        idx = np.full((B, S, K), N - 3, np.int32)
    else:
        idx = rng.integers(0, N + 1, size=(B, S, K)).astype(np.int32)      # N: the empty-row value
        idx[0, 0] = N
    return xyz, new, pts, idx


@pytest.mark.parametrize("D", [0, 5, 64, 131])
def test_group_fwd_bitwise(G, dev, D):
    xyz, new, pts, idx = _group_case(D, 10 + D)
    got = G.GroupFn.apply(_t(xyz, dev), _t(new, dev), None if pts is None else _t(pts, dev), _t(idx, dev))
    want = R.group_fwd(xyz, new, pts, idx)
    assert tuple(got.shape) == want.shape
    assert (got.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    assert (want[idx.reshape(-1) == 100] == 0).all()
    if D:                                             # the plain gather (index_points)
        got = G.GroupFn.apply(None, None, _t(pts, dev), _t(idx, dev))
        assert (got.cpu().numpy().view(np.uint32) == R.group_fwd(None, None, pts, idx).view(np.uint32)).all()


def _check_bwd(got, ref64, asum, n, what):
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref64)
    bound = (n + 1) * U * asum
    worst = (err - bound).max()
    print(f"{what}: max err {err.max():.3e}, max n_e {int(n.max())}, worst err - bound {worst:.3e}")
    assert (err <= bound).all(), f"{what}: an element misses (n_e + 1) * 2^-24 * sum|terms| by {worst:.3e}"


@pytest.mark.parametrize("D,degenerate", [(0, False), (5, False), (64, False), (131, False), (5, True), (70, True)])
def test_group_bwd_bound_and_determinism(G, dev, D, degenerate):
    B, N, S, K = (2, 100, 9, 7) if not degenerate else (2, 150, 40, 16)
    xyz, new, pts, idx = _group_case(D, 30 + D, B, N, S, K, degenerate)
    rng = np.random.default_rng(50 + D)
    g = rng.standard_normal((B * S * K, 3 + D)).astype(np.float32)
    r = R.group_bwd(g, idx, N, 3)
    if degenerate:
        assert r["n"].max() == S * K
    runs = []
    for _ in range(2):
        x, c = _t(xyz, dev).requires_grad_(True), _t(new, dev).requires_grad_(True)
        p = None if pts is None else _t(pts, dev).requires_grad_(True)
        out = G.GroupFn.apply(x, c, p, _t(idx, dev))
        out.backward(_t(g, dev))
        runs.append((x.grad, c.grad, None if p is None else p.grad))
    for a, b in zip(*runs):
        assert a is None and b is None or torch.equal(a, b)
    gx, gn, gp = runs[0]
    _check_bwd(gx, r["gx"], r["ax"], r["n"][..., None], "grad_xyz")
    _check_bwd(gn, r["gn"], r["an"], r["nn"][..., None], "grad_new_xyz")
    if D:
        _check_bwd(gp, r["gp"], r["ap"], r["n"][..., None], "grad_points")


def test_group_autograd_wiring(G, dev):
    xyz, new, pts, idx = _group_case(4, 77)
    i = _t(idx, dev)
    # points alone (the gather form): only points gets a gradient, written in full
    p = _t(pts, dev).requires_grad_(True)
    out = G.GroupFn.apply(None, None, p, i)
    assert out.requires_grad and tuple(out.shape) == (idx.size, 4)
    out.sum().backward()
    cnt = R.group_bwd(np.ones((idx.size, 4), np.float32), idx, 100, 0)["gp"]
    np.testing.assert_array_equal(p.grad.cpu().numpy(), cnt.astype(np.float32))
    # points=None: xyz and new_xyz only; a constant input gets no gradient; idx never does
    x, c = _t(xyz, dev).requires_grad_(True), _t(new, dev)
    out = G.GroupFn.apply(x, c, None, i)
    assert tuple(out.shape) == (idx.size, 3)
    out.sum().backward()
    assert x.grad is not None and c.grad is None and i.grad is None
    with pytest.raises(ValueError, match="int32"):
        G.GroupFn.apply(x, c, None, i.long())
    with pytest.raises(ValueError, match="go together"):
        G.GroupFn.apply(x, None, None, i)


def test_utils_match_the_reference_outputs(dev, gold, built):
    """index_points / sample_and_group with the reference's signatures and dtypes, on the golden."""
    from network.pointnet import pointnet2_utils as P
    xyz, pts, start = _t(gold["sa_xyz"], dev), _t(gold["sa_points"], dev), _t(gold["sa_start"], dev)
    nx, npts, gxyz, fidx = P.sample_and_group(SA["npoint"], SA["radius"], SA["nsample"], xyz, pts, returnfps=True,
                                              start=start)
    assert fidx.dtype == torch.long
    np.testing.assert_array_equal(fidx.cpu().numpy(), gold["sg_fps_idx"])
    for got, k in ((nx, "sg_new_xyz"), (npts, "sg_new_points"), (gxyz, "sg_grouped_xyz")):
        np.testing.assert_array_equal(got.cpu().numpy(), gold[k])
    idx = P.query_ball_point(SA["radius"], SA["nsample"], xyz, nx)
    assert idx.dtype == torch.long
    np.testing.assert_array_equal(idx.cpu().numpy(), gold["sg_idx"])
    assert P.farthest_point_sample(xyz, 8, start).dtype == torch.long
    np.testing.assert_array_equal(P.index_points(xyz, fidx).cpu().numpy(), gold["sg_new_xyz"])      # idx [B,S]
    np.testing.assert_array_equal(P.index_points(pts, idx).cpu().numpy(), gold["sg_new_points"][..., 3:])
    nz, allp = P.sample_and_group_all(xyz, pts)
    assert tuple(nz.shape) == (2, 1, 3) and not nz.any() and tuple(allp.shape) == (2, 1, 256, 8)
    np.testing.assert_array_equal(allp[:, 0, :, :3].cpu().numpy(), gold["sa_xyz"])


# ---------------- the set-abstraction layer ----------------

def _sd(gold):
    return {k[len("sa_sd_"):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("sa_sd_")}


def _inputs(gold):
    return (np.ascontiguousarray(gold["sa_xyz"].transpose(0, 2, 1)), np.ascontiguousarray(gold["sa_points"].transpose(0, 2, 1)))


@pytest.fixture(scope="module")
def ref32(gold):
    x, p = _inputs(gold)
    sd = {k: v.numpy() for k, v in _sd(gold).items()}
    return R.sa_layer(sd, x, p, gold["sa_start"], SA["npoint"], SA["radius"], SA["nsample"], False, torch.float32,
                      gold["sa_g_out"], gold["sa_g_xyz"])


def _tol(r32, r64, f):
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    return 3.0 * np.abs(r32 - r64).max() + f * np.abs(r64).max()


def _close(got, r32, r64, f, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    err, tol = np.abs(got - r64).max(), _tol(r32, r64, f)
    print(f"{what:28s} err {err:.3e} (allowed {tol:.3e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _run_layer(gold, dev):
    from network.pointnet.pointnet2_utils import PointNetSetAbstraction
    layer = PointNetSetAbstraction(SA["npoint"], SA["radius"], SA["nsample"], 3 + 5, [16, 32], False)
    layer.load_state_dict(_sd(gold), strict=True)
    layer.to(dev).train()
    xn, pn = _inputs(gold)
    x, p = _t(xn, dev).requires_grad_(True), _t(pn, dev).requires_grad_(True)
    new_xyz, out = layer(x, p, start=_t(gold["sa_start"], dev))
    ((out * _t(gold["sa_g_out"], dev)).sum() + (new_xyz * _t(gold["sa_g_xyz"], dev)).sum()).backward()
    return layer, x, p, new_xyz, out


def test_sa_layer_train_step_vs_golden(dev, gold, ref32):
    layer, x, p, new_xyz, out = _run_layer(gold, dev)
    assert tuple(out.shape) == (2, 32, SA["npoint"]) and tuple(new_xyz.shape) == (2, 3, SA["npoint"])
    np.testing.assert_array_equal(new_xyz.detach().cpu().numpy(), gold["sa_ref_new_xyz"].astype(np.float32))
    _close(out, ref32["out"], gold["sa_ref_out"], F_FWD, "out")
    _close(x.grad, ref32["gxyz"], gold["sa_ref_gxyz"], F_GRAD, "grad xyz")
    _close(p.grad, ref32["gpoints"], gold["sa_ref_gpoints"], F_GRAD, "grad points")
    for k, v in layer.named_parameters():
        r64 = gold[f"sa_grad_{k}"]
        if k.startswith("mlp_convs") and k.endswith("bias"):      # zero true gradient
            dW = gold[f"sa_grad_{k[:-4]}weight"]
            got, lim = v.grad.abs().max().item(), 3.0 * np.abs(ref32["grads"][k]).max() + 1e-5 * np.abs(dW).max()
            print(f"{k:28s} zero-gradient bias {got:.3e} (allowed {lim:.3e})")
            assert got <= lim, k
        else:
            _close(v.grad, ref32["grads"][k], r64, F_GRAD, k)
    for k, v in layer.state_dict().items():
        if "running" in k:
            _close(v, ref32["running"][k], gold[f"sa_after_{k}"], F_FWD, k)
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1


def test_sa_layer_second_run_is_bitwise_equal(dev, gold):
    a, b = _run_layer(gold, dev), _run_layer(gold, dev)
    assert torch.equal(a[4], b[4]) and torch.equal(a[1].grad, b[1].grad) and torch.equal(a[2].grad, b[2].grad)
    for (k, v), (_, w) in zip(a[0].named_parameters(), b[0].named_parameters()):
        assert torch.equal(v.grad, w.grad), k
    for (k, v), (_, w) in zip(a[0].state_dict().items(), b[0].state_dict().items()):
        assert torch.equal(v, w), k


def test_sa_layer_group_all(dev, gold):
    """group_all: one group of all N points, new_xyz zeros; vs the restatement in float64 / float32 on
    the first 249 points of the golden cloud (a count at which, with the golden weights, every ReLU
    and max-pool decision is clear of twice the forward tolerance in float64: asserted first)."""
    from network.pointnet.pointnet2_utils import PointNetSetAbstraction
    xn, pn = (a[:, :, :249].copy() for a in _inputs(gold))
    sd = {k: v.numpy() for k, v in _sd(gold).items()}
    g_out = gold["sa_g_out"][:, :, :1]
    r64, r32 = (R.sa_layer(sd, xn, pn, None, None, None, None, True, dt, g_out, None) for dt in (torch.float64, torch.float32))
    assert min(R.decision_margin(r64["pre"])) > 2 * _tol(r32["out"], r64["out"], F_FWD)
    layer = PointNetSetAbstraction(None, None, None, 3 + 5, [16, 32], True)
    layer.load_state_dict(_sd(gold), strict=True)
    layer.to(dev).train()
    x, p = _t(xn, dev).requires_grad_(True), _t(pn, dev).requires_grad_(True)
    new_xyz, out = layer(x, p)
    assert tuple(new_xyz.shape) == (2, 3, 1) and not new_xyz.any() and tuple(out.shape) == (2, 32, 1)
    _close(out, r32["out"], r64["out"], F_FWD, "group_all out")
    (out * _t(g_out, dev)).sum().backward()
    _close(x.grad, r32["gxyz"], r64["gxyz"], F_GRAD, "group_all grad xyz")
    _close(p.grad, r32["gpoints"], r64["gpoints"], F_GRAD, "group_all grad points")
    for k, v in layer.named_parameters():
        if not (k.startswith("mlp_convs") and k.endswith("bias")):
            _close(v.grad, r32["grads"][k], r64["grads"][k], F_GRAD, "group_all " + k)


def test_sa_layer_graph_capture(dev, gold):
    """Forward (training-mode BN) captured in a graph with a given start and replayed on new inputs:
    equal to the eager run. A host read anywhere in the layer would fail the capture."""
    from network.pointnet.pointnet2_utils import PointNetSetAbstraction
    layer = PointNetSetAbstraction(SA["npoint"], SA["radius"], SA["nsample"], 3 + 5, [16, 32], False)
    layer.load_state_dict(_sd(gold), strict=True)
    layer.to(dev).train()
    xn, pn = _inputs(gold)
    x, p, start = _t(xn, dev), _t(pn, dev), _t(gold["sa_start"], dev)
    with torch.no_grad():
        layer(x, p, start=start)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            new_xyz, out = layer(x, p, start=start)
        rng = np.random.default_rng(3)
        x.copy_(_t(_grid(rng, 2, 256, 8).transpose(0, 2, 1), dev))
        p.copy_(_t(rng.standard_normal((2, 5, 256)).astype(np.float32), dev))
        start.copy_(torch.tensor([5, 200], device=dev, dtype=start.dtype))
        g.replay()
        torch.cuda.synchronize()
        e_xyz, e_out = layer(x, p, start=start)
    assert torch.equal(new_xyz, e_xyz) and torch.equal(out, e_out)
    want = R.fps(np.ascontiguousarray(x.cpu().numpy().transpose(0, 2, 1)), [5, 200], SA["npoint"])
    np.testing.assert_array_equal(e_xyz.cpu().numpy(), x.cpu().numpy()[np.arange(2)[:, None, None], np.arange(3)[None, :, None],
                                                                      want[:, None, :]])
