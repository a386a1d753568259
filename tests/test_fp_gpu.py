"""Feature propagation and multi-scale grouping on the GPU (csrc/interp.hip, ured_hip/interp.py,
network/pointnet/pointnet2_utils.py) against tests/fp_ref.py and tests/golden/fp.npz.

Kernel level (u = 2^-24; every bound is checked per element against float64, and the fp32 numpy
restatement is held to the same bounds on the CPU by tests/test_fp_ref.py):
  three_nn      bitwise equal to the restatement, distances and indices.
  forward       |err| <= 10 u sum_k |w_k f_kc|: nine roundings on the path (add, reciprocal, two for
                R, divide, product, two for the sum, the comparison's own), each at most u relative
                to a quantity bounded by sum_k |w_k f_kc| (1 + u)^9. The points1 columns are a copy.
  grad_points2  |err| <= (n_e + 8) u sum|terms|, n_e the element's term count: the sequential-sum
                bound of tests/test_group_gpu.py (n_e + 1) plus one product and the weight's five
                roundings. Two runs are bitwise equal.
  grad_d2       finite and |err| <= (D2 + 16) u T_e, T_e = r_k w_k sum_{j != k} w_j sum_c |g_c|
                (|f_kc| + |f_jc|): D2 for the dot products in any summation order, the rest for the
                weights, r_k, the differences, the products and the outer sum.
  grad_points1  bitwise the first D1 columns of g.

Layer level: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|, f = 1e-5 forward and running
statistics, 2e-5 gradients (the idiom of tests/test_group_gpu.py), ref64 the golden (the reference's
own layer in float64), ref32 the fp_ref layer in float32 on the CPU; a conv bias in front of
training-mode BN has a zero true gradient and is bounded as there. tests/test_fp_ref.py asserts that
no ReLU / max-pool decision of the golden layers lies within twice the forward tolerance and that
the third neighbour of every query is clear of the fourth. Nothing is derived from the GPU's output.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import fp_ref as R
from conftest import GOLDEN
from fp_ref import CASES, MSG, bcn, fp_ref_layer, msg_ref_layer, sd_of

pytestmark = pytest.mark.gpu
F_FWD, F_GRAD = 1e-5, 2e-5


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "fp.npz")))


@pytest.fixture(scope="module")
def I(dev):
    from ured_hip import interp
    return interp


@pytest.fixture(autouse=True)
def _interp_debug_word():
    """The debug build's bounds word of interp.hip (file id 13), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_interp"):
        return
    fn = mod._lib.ured_dbg_interp
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): interp.hip:{v & 0xFFFFFFFF}"


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------- kernel level ----------------

@pytest.mark.parametrize("B,N,S,D2,D1,coincident", CASES)
def test_interp_kernels_vs_float64(I, dev, B, N, S, D2, D1, coincident):
    """three_nn, forward, the three gradients and the second run of one case (bounds: module docstring)."""
    c = R.kernel_case(B, N, S, D2, D1, coincident)
    K = min(3, S)
    runs = []
    for _ in range(2):
        x1, x2 = _t(c["xyz1"], dev), _t(c["xyz2"], dev)
        d2, idx = I.three_nn(x1, x2)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, N, K)
        np.testing.assert_array_equal(idx.cpu().numpy(), c["idx"])
        assert (d2.cpu().numpy().view(np.uint32) == c["d2"].view(np.uint32)).all()
        p1 = None if D1 == 0 else _t(c["points1"], dev).requires_grad_(True)
        p2 = _t(c["points2"], dev).requires_grad_(True)
        dd = d2.detach().requires_grad_(True)
        out = I.InterpFn.apply(p1, p2, idx, dd)
        assert tuple(out.shape) == (B * N, D1 + D2)
        out.backward(_t(c["g"], dev))
        runs.append((out.detach(), p2.grad, dd.grad, None if p1 is None else p1.grad))
    for a, b in zip(*runs):
        assert a is None and b is None or torch.equal(a, b)
    out, gp2, gd2, gp1 = (None if a is None else a.cpu().numpy() for a in runs[0])
    R.check_fwd(out, c)
    R.check_bwd(gp2, gd2, c)
    if D1:
        assert (gp1.view(np.uint32) == c["g"].reshape(B, N, -1)[..., :D1].view(np.uint32)).all()
    if K == 1:                                        # bitwise the broadcast of the one coarse row
        want = np.repeat(c["points2"], N, axis=1).reshape(B * N, D2)
        assert (out[:, D1:].view(np.uint32) == want.view(np.uint32)).all()
        assert not gd2.any()


def test_interp_vectorised_and_scalar_paths_agree(I, dev):
    """D1 = 8, D2 = 64 takes the four-channel path, the same data at an odd split (D1 = 7, D2 = 65:
    the last points1 column moved to the front of points2's) the scalar one; each meets the forward
    bound, and the interpolated columns they share are bitwise equal."""
    c = R.kernel_case(2, 130, 40, 64, 8)
    x = [_t(c[k], dev) for k in ("points1", "points2")]
    i, d = _t(c["idx"], dev), _t(c["d2"], dev)
    out = I.InterpFn.apply(x[0], x[1], i, d).cpu().numpy()
    R.check_fwd(out, c)
    odd = dict(c, points1=c["points1"][..., :7].copy(), D1=7,
               points2=np.concatenate([c["points2"][..., :1], c["points2"]], -1))
    out2 = I.InterpFn.apply(_t(odd["points1"], dev), _t(odd["points2"], dev), i, d).cpu().numpy()
    R.check_fwd(out2, odd)
    assert (out2[:, 8:].view(np.uint32) == out[:, 8:].view(np.uint32)).all()


def test_interp_gradient_reaches_both_clouds(I, dev):
    """d2's gradient flows on into knn's backward: against the float64 chain rule
    grad_xyz1[n] = sum_k 2 gd2[n,k] (x1_n - x2_idx), grad_xyz2 its scatter, with gd2 the float64
    weight gradient. Bound: the (D2 + 16) u T_e of grad_d2 carried through |2 (x1 - x2)| per term, plus
    (n_e + 3) u sum|terms| for knn's own products and sequential sum."""
    c = R.kernel_case(2, 256, 64, 37, 0)
    B, N, S, D2 = 2, 256, 64, 37
    x1, x2 = _t(c["xyz1"], dev).requires_grad_(True), _t(c["xyz2"], dev).requires_grad_(True)
    d2, idx = I.three_nn(x1, x2)
    I.InterpFn.apply(None, _t(c["points2"], dev), idx, d2).backward(_t(c["g"], dev))
    r = R.interp_bwd64(c["g"], c["points2"], c["idx"], c["d2"], 0)
    X1, X2 = c["xyz1"].astype(np.float64), c["xyz2"].astype(np.float64)
    diff = 2.0 * (X1[:, :, None, :] - X2[np.arange(B)[:, None, None], c["idx"]])        # [B,N,K,3]
    term, tb = r["gd2"][..., None] * diff, ((D2 + R.C_GD2) * R.U * r["Te"])[..., None] * np.abs(diff)
    g1, a1, e1 = term.sum(2), np.abs(term).sum(2), tb.sum(2)
    g2, a2, e2, n2 = np.zeros((B, S, 3)), np.zeros((B, S, 3)), np.zeros((B, S, 3)), np.zeros((B, S, 1))
    for b in range(B):
        j = c["idx"][b].reshape(-1).astype(np.int64)
        np.add.at(g2[b], j, -term[b].reshape(-1, 3))
        np.add.at(a2[b], j, np.abs(term[b]).reshape(-1, 3))
        np.add.at(e2[b], j, tb[b].reshape(-1, 3))
        np.add.at(n2[b], j, 1)
    for got, ref, asum, carried, n, what in ((x1.grad, g1, a1, e1, 3, "grad_xyz1"), (x2.grad, g2, a2, e2, n2, "grad_xyz2")):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        bound = carried + (n + 3) * R.U * asum
        print(f"{what}: max err {err.max():.3e}, worst err - bound {(err - bound).max():.3e}")
        assert (err <= bound).all(), what


def test_interp_autograd_wiring(I, dev):
    c = R.kernel_case(2, 200, 3, 5, 6)
    idx, d2 = _t(c["idx"], dev), _t(c["d2"], dev)
    # points1=None: the interpolation alone; a constant input gets no gradient; idx never does
    p2 = _t(c["points2"], dev).requires_grad_(True)
    out = I.InterpFn.apply(None, p2, idx, d2)
    assert out.requires_grad and tuple(out.shape) == (400, 5)
    out.sum().backward()
    assert p2.grad is not None and d2.grad is None and idx.grad is None
    p1 = _t(c["points1"], dev).requires_grad_(True)
    out = I.InterpFn.apply(p1, p2.detach(), idx, d2)
    assert tuple(out.shape) == (400, 11)
    out.backward(_t(c["g"][:400, :11], dev))
    assert (p1.grad.cpu().numpy() == c["g"][:400, :6].reshape(2, 200, 6)).all()
    with pytest.raises(ValueError, match="int32"):
        I.InterpFn.apply(None, p2, idx.long(), d2)
    with pytest.raises(ValueError, match=r"K 4 outside \[1, 3\]"):
        I.InterpFn.apply(None, p2, torch.zeros(2, 200, 4, dtype=torch.int32, device=dev), torch.zeros(2, 200, 4, device=dev))
    with pytest.raises(ValueError, match="d2 must be float32"):
        I.InterpFn.apply(None, p2, idx, d2[:, :, :2])
    with pytest.raises(ValueError, match="points1 has 100 rows"):
        I.InterpFn.apply(p1[:, :100], p2, idx, d2)
    d, i = I.three_nn(_t(c["xyz1"], dev), _t(c["xyz2"][:, :2], dev))       # never more columns than S
    assert tuple(d.shape) == (2, 200, 2) and tuple(i.shape) == (2, 200, 2)


# ---------------- layer level ----------------

def _tol(r32, r64, f):
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    return 3.0 * np.abs(r32 - r64).max() + f * np.abs(r64).max()


def _close(got, r32, r64, f, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    err, tol = np.abs(got - r64).max(), _tol(r32, r64, f)
    print(f"{what:32s} err {err:.3e} (allowed {tol:.3e})")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _check_params(layer, gold, tag, ref32, conv_prefix):
    for k, v in layer.named_parameters():
        r64 = gold[f"{tag}_grad_{k}"]
        if k.startswith(conv_prefix) and k.endswith("bias"):      # zero true gradient
            dW = gold[f"{tag}_grad_{k[:-4]}weight"]
            got, lim = v.grad.abs().max().item(), 3.0 * np.abs(ref32["grads"][k]).max() + 1e-5 * np.abs(dW).max()
            print(f"{k:32s} zero-gradient bias {got:.3e} (allowed {lim:.3e})")
            assert got <= lim, k
        else:
            _close(v.grad, ref32["grads"][k], r64, F_GRAD, k)
    for k, v in layer.state_dict().items():
        if "running" in k:
            _close(v, ref32["running"][k], gold[f"{tag}_after_{k}"], F_FWD, k)
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1


FP_CFG = {"fpa": (16, [32, 16]), "fpb": (12, [16])}


def _fp_layer(gold, tag, dev):
    from network.pointnet.pointnet2_utils import PointNetFeaturePropagation
    layer = PointNetFeaturePropagation(*FP_CFG[tag])
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd_of(gold, tag).items()}, strict=True)
    return layer.to(dev).train()


def _fp_inputs(gold, tag, dev):
    return [None if a is None else _t(bcn(a), dev).requires_grad_(True)
            for a in (gold[f"{tag}_xyz1"], gold[f"{tag}_xyz2"], gold.get(f"{tag}_points1"), gold[f"{tag}_points2"])]


def _run_fp(gold, tag, dev):
    layer, ins = _fp_layer(gold, tag, dev), _fp_inputs(gold, tag, dev)
    out = layer(*ins)
    (out * _t(gold[f"{tag}_g_out"], dev)).sum().backward()
    return layer, ins, out


@pytest.fixture(scope="module")
def fp_ref32(gold):
    return {tag: fp_ref_layer(gold, tag, torch.float32) for tag in FP_CFG}


@pytest.mark.parametrize("tag", ["fpa", "fpb"])
def test_fp_layer_train_step_vs_golden(dev, gold, fp_ref32, tag):
    """Case a: N = 192 from an FPS subset of 48, with skip features; case b: S = 1 (the K = 1 path, no
    neighbour search, no coordinate gradient), no skip features."""
    ref32 = fp_ref32[tag]
    layer, (x1, x2, p1, p2), out = _run_fp(gold, tag, dev)
    assert tuple(out.shape) == gold[f"{tag}_ref_out"].shape
    _close(out, ref32["out"], gold[f"{tag}_ref_out"], F_FWD, "out")
    _close(p2.grad, ref32["gpoints2"], gold[f"{tag}_ref_gpoints2"], F_GRAD, "grad points2")
    if tag == "fpa":
        _close(p1.grad, ref32["gpoints1"], gold["fpa_ref_gpoints1"], F_GRAD, "grad points1")
        _close(x1.grad, ref32["gxyz1"], gold["fpa_ref_gxyz1"], F_GRAD, "grad xyz1")
        _close(x2.grad, ref32["gxyz2"], gold["fpa_ref_gxyz2"], F_GRAD, "grad xyz2")
    else:
        assert x1.grad is None and x2.grad is None and not gold["fpb_ref_gxyz1"].any()
    _check_params(layer, gold, tag, ref32, "mlp_convs")


@pytest.mark.parametrize("tag", ["fpa", "fpb"])
def test_fp_layer_second_run_is_bitwise_equal(dev, gold, tag):
    a, b = _run_fp(gold, tag, dev), _run_fp(gold, tag, dev)
    assert torch.equal(a[2], b[2])
    for u, v in zip(a[1], b[1]):
        assert u is None and v is None or u.grad is None and v.grad is None or torch.equal(u.grad, v.grad)
    for (k, v), (_, w) in zip(a[0].named_parameters(), b[0].named_parameters()):
        assert torch.equal(v.grad, w.grad), k
    for (k, v), (_, w) in zip(a[0].state_dict().items(), b[0].state_dict().items()):
        assert torch.equal(v, w), k


def test_fp_layer_two_coarse_points(dev, gold, fp_ref32):
    """S = 2 interpolates over two neighbours, as the reference's [:, :, :3] slice does: the first two
    coarse points of case a, against the restatement in float64 / float32 (decisions asserted clear)."""
    sd = sd_of(gold, "fpa")
    args = [bcn(gold["fpa_xyz1"]), bcn(gold["fpa_xyz2"][:, :2]), bcn(gold["fpa_points1"]), bcn(gold["fpa_points2"][:, :2])]
    r64, r32 = (R.fp_layer(sd, *args, dt, gold["fpa_g_out"]) for dt in (torch.float64, torch.float32))
    assert r64["idx"].shape == (2, 192, 2)
    assert R.relu_margin(r64["pre"]) > 2 * _tol(r32["out"], r64["out"], F_FWD)
    layer = _fp_layer(gold, "fpa", dev)
    ins = [_t(a, dev).requires_grad_(True) for a in args]
    out = layer(*ins)
    _close(out, r32["out"], r64["out"], F_FWD, "S=2 out")
    (out * _t(gold["fpa_g_out"], dev)).sum().backward()
    for t, k in zip(ins, ("gxyz1", "gxyz2", "gpoints1", "gpoints2")):
        _close(t.grad, r32[k], r64[k], F_GRAD, "S=2 " + k)


def test_fp_layer_graph_capture(dev, gold):
    """Forward (training-mode BN) captured in a graph and replayed on new inputs: equal to the eager
    run. A host read anywhere in the layer would fail the capture."""
    layer = _fp_layer(gold, "fpa", dev)
    ins = [t.detach() for t in _fp_inputs(gold, "fpa", dev)]
    with torch.no_grad():
        layer(*ins)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = layer(*ins)
        rng = np.random.default_rng(3)
        for t in ins:
            t.copy_(_t(rng.standard_normal(tuple(t.shape)).astype(np.float32), dev))
        g.replay()
        torch.cuda.synchronize()
        eager = layer(*ins)
    assert torch.equal(out, eager)


def _msg_layer(gold, dev, D=5):
    from network.pointnet.pointnet2_utils import PointNetSetAbstractionMsg
    layer = PointNetSetAbstractionMsg(MSG["npoint"], MSG["radius_list"], MSG["nsample_list"], D, [[16, 32], [16, 24]])
    if D == 5:
        layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd_of(gold, "msg").items()}, strict=True)
    return layer.to(dev).train()


def _run_msg(gold, dev):
    layer = _msg_layer(gold, dev)
    x, p = (_t(bcn(gold[k]), dev).requires_grad_(True) for k in ("msg_xyz", "msg_points"))
    new_xyz, out = layer(x, p, start=_t(gold["msg_start"], dev))
    ((out * _t(gold["msg_g_out"], dev)).sum() + (new_xyz * _t(gold["msg_g_xyz"], dev)).sum()).backward()
    return layer, x, p, new_xyz, out


def test_msg_layer_train_step_vs_golden(dev, gold):
    ref32 = msg_ref_layer(gold, torch.float32)
    layer, x, p, new_xyz, out = _run_msg(gold, dev)
    assert tuple(out.shape) == (2, 32 + 24, MSG["npoint"]) and tuple(new_xyz.shape) == (2, 3, MSG["npoint"])
    np.testing.assert_array_equal(new_xyz.detach().cpu().numpy(), gold["msg_ref_new_xyz"].astype(np.float32))
    _close(out, ref32["out"], gold["msg_ref_out"], F_FWD, "out")
    _close(x.grad, ref32["gxyz"], gold["msg_ref_gxyz"], F_GRAD, "grad xyz")
    _close(p.grad, ref32["gpoints"], gold["msg_ref_gpoints"], F_GRAD, "grad points")
    _check_params(layer, gold, "msg", ref32, "conv_blocks")


def test_msg_layer_second_run_is_bitwise_equal(dev, gold):
    a, b = _run_msg(gold, dev), _run_msg(gold, dev)
    assert torch.equal(a[4], b[4]) and torch.equal(a[1].grad, b[1].grad) and torch.equal(a[2].grad, b[2].grad)
    for (k, v), (_, w) in zip(a[0].named_parameters(), b[0].named_parameters()):
        assert torch.equal(v.grad, w.grad), k
    for (k, v), (_, w) in zip(a[0].state_dict().items(), b[0].state_dict().items()):
        assert torch.equal(v, w), k


def test_msg_layer_without_points(dev, gold):
    """points=None (rows are xyz - centre alone, no column rotation): against the restatement in
    float64 / float32 with the layer's own seeded weights. Seed 8 is one of the first twenty that keep
    every ReLU and max-pool decision clear of twice the forward tolerance in float64 (found on the
    CPU); that is asserted before anything runs on the device."""
    torch.manual_seed(8)
    layer = _msg_layer(gold, dev, D=0)
    sd = {k: v.cpu().numpy() for k, v in layer.state_dict().items()}
    C = 32 + 24
    args = (bcn(gold["msg_xyz"]), None, gold["msg_start"], MSG["npoint"], MSG["radius_list"], MSG["nsample_list"])
    r64, r32 = (R.msg_layer(sd, *args, dt, gold["msg_g_out"][:, :C], gold["msg_g_xyz"]) for dt in (torch.float64, torch.float32))
    import group_ref as GR
    tol = _tol(r32["out"], r64["out"], F_FWD)
    margins = [GR.decision_margin(p) for p in r64["pre"]]
    assert min(m[0] for m in margins) > 2 * tol and min(m[1] for m in margins) > 2 * tol, (margins, tol)
    x = _t(bcn(gold["msg_xyz"]), dev).requires_grad_(True)
    new_xyz, out = layer(x, None, start=_t(gold["msg_start"], dev))
    np.testing.assert_array_equal(new_xyz.detach().cpu().numpy(), r64["new_xyz"].astype(np.float32))
    _close(out, r32["out"], r64["out"], F_FWD, "no-points out")
    ((out * _t(gold["msg_g_out"][:, :C], dev)).sum() + (new_xyz * _t(gold["msg_g_xyz"], dev)).sum()).backward()
    _close(x.grad, r32["gxyz"], r64["gxyz"], F_GRAD, "no-points grad xyz")
    for k, v in layer.named_parameters():
        if not (k.startswith("conv_blocks") and k.endswith("bias")):
            _close(v.grad, r32["grads"][k], r64["grads"][k], F_GRAD, "no-points " + k)
