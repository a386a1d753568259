"""The DCD training loss on the GPU (csrc/dcd.hip, ured_hip/dcd.py, the routing of
chamfer3D.model_utils.calc_dcd and ured_hip.nn.dcd) against tests/dcd_loss_ref.py in float64, which
tests/test_dcd_loss_ref.py pins to the reference's own calc_dcd and its autograd gradient.

Per case: the NN indices bit for bit against oracle.nn_ref (so the restatement runs under the GPU's
decisions), the loss within 2e-6 (tests/test_pairs_gpu.py), the gradients within tests/tol_check.py:
err(gpu, ref64) <= 3 * err(ref32, ref64) + 2e-5 * max|ref64| with ref32 the same restatement in
float32 on the CPU, and a second backward bit for bit. Nothing is derived from the GPU's output.
The point counts lie on either side of the wave (64), the workgroup (256) and the 1024-entry LDS
tile of the backward; (2, 8192, 8192) is exactly the limit of 16384 points per pair.
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import dcd_loss_ref as R
from oracle import nn_ref
from tol_check import F_GRAD, check

pytestmark = pytest.mark.gpu
WORST = {}
TOL = 2e-6


@pytest.fixture(scope="module")
def D(dev):
    from ured_hip import dcd
    yield dcd
    for fam, (ratio, what) in sorted(WORST.items()):
        print(f"worst ratio {fam:14s} {ratio:.3f}  ({what})")


@pytest.fixture(autouse=True)
def _dcd_debug_word():
    """The debug build's bounds word of dcd.hip (file id 16), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_dcd"):
        return
    fn = mod._lib.ured_dbg_dcd
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): dcd.hip:{v & 0xFFFFFFFF}"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _run_case(D, dev, x, gt, alpha, lam, nr, cot, what, wrt=("x", "gt"), expect_zero_grad=False):
    """cot: name of an output (loss, cd_t, dist1, dist2) -> numpy cotangent."""
    o = nn_ref.nn_fwd(gt, x)
    xg = _t(x).to(dev).requires_grad_("x" in wrt)
    gg = _t(gt).to(dev).requires_grad_("gt" in wrt)

    def once():
        xg.grad = gg.grad = None
        loss, d1, d2, i1, i2 = D.dcd_loss(xg, gg, alpha=alpha, n_lambda=lam, non_reg=nr)
        outs = {"loss": loss, "dist1": d1, "dist2": d2, "cd_t": d1.mean(1) + d2.mean(1)}
        sum((outs[k] * _t(v).float().to(dev)).sum() for k, v in cot.items()).backward()
        return loss, d1, d2, i1, i2, xg.grad, gg.grad

    loss, d1, d2, i1, i2, gx, ggt = once()
    assert not i1.requires_grad and not i2.requires_grad
    assert (i1.cpu().numpy() == o[2]).all() and (i2.cpu().numpy() == o[3]).all(), f"{what}: NN idx differ from the oracle"
    r64, g64 = R.run(x, gt, o[2], o[3], alpha, lam, nr, cot=cot, wrt=wrt)
    r32, g32 = R.run(x, gt, o[2], o[3], alpha, lam, nr, cot=cot, wrt=wrt, dtype=torch.float32)
    err = (loss.detach().double().cpu() - r64["loss"]).abs().max().item()
    print(f"{what}: loss err {err:.3e}")
    assert err <= TOL, f"{what}: loss {err:.3e} off float64"
    for name, g in (("x", gx), ("gt", ggt)):
        if name not in wrt:
            assert g is None, f"{what}: a gradient for {name}, which requires none"
            continue
        check(WORST, "dcd_loss_bwd", f"{what} d{name}", g, g32[name], g64[name], F_GRAD)
        if expect_zero_grad:
            assert bool((g == 0).all()), f"{what}: d{name} not exactly zero"
    again = once()
    assert torch.equal(loss, again[0]), f"{what}: two forwards differ"
    for a, b in ((gx, again[5]), (ggt, again[6])):
        assert (a is None and b is None) or torch.equal(a, b), f"{what}: two backwards differ"
    return loss, d1, d2


SHAPES = [(1, 1, 1), (3, 63, 65), (2, 300, 200), (2, 257, 1025), (1, 1100, 64), (2, 8192, 8192)]


@pytest.mark.parametrize("i,shape", list(enumerate(SHAPES)))
def test_shapes(D, dev, i, shape):
    b, n_x, n_gt = shape
    alpha, lam, nr = R.PARAMS[i % len(R.PARAMS)]
    x, gt = R.make_inputs(100 + i, b, n_x, n_gt)
    _run_case(D, dev, x, gt, alpha, lam, nr, {"loss": R.cotangent(b)}, f"{b}x{n_x}x{n_gt} a{alpha} l{lam}")


@pytest.mark.parametrize("lam", [0, 0.5, 1, 2, 1.5])
@pytest.mark.parametrize("nr", [False, True])
def test_lambdas_and_non_reg(D, dev, lam, nr):
    x, gt = R.make_inputs(7, 2, 300, 200)
    _run_case(D, dev, x, gt, 200, lam, nr, {"loss": R.cotangent(2)}, f"2x300x200 l{lam} nr{int(nr)}")


def test_every_gt_point_visits_one_x_point(D, dev):
    """count = n_gt for x point 0; the other x points are far from every gt point."""
    x, gt = R.make_inputs(21, 2, 130, 300)
    x = x + np.float32(10.0)
    x[:, 0] = 0.5
    assert (nn_ref.nn_fwd(gt, x)[2] == 0).all()
    _run_case(D, dev, x, gt, 40, 1, False, {"loss": R.cotangent(2)}, "one visited point")


def test_exact_duplicates(D, dev):
    """d = 0 for the copied points: loss and cd_t are differentiable there (cd_p is not)."""
    x, gt = R.make_inputs(22, 2, 200, 200)
    x[:, :150] = gt[:, 50:]
    x[:, 150:160] = gt[:, :10]           # duplicates inside x as well (ties: lowest index)
    _run_case(D, dev, x, gt, 1000, 1, False, {"loss": R.cotangent(2), "cd_t": R.cotangent(2, 0.3)}, "duplicates")


def test_exp_underflow_gives_zero_gradient(D, dev):
    x, gt = R.make_inputs(23, 2, 70, 90)
    x = x + np.float32(3.0)               # every distance > 4: exp(-1e3 d) underflows to 0
    loss, _, _ = _run_case(D, dev, x, gt, 1000, 1, False, {"loss": R.cotangent(2)}, "underflow", expect_zero_grad=True)
    assert bool((loss == 1).all())


def test_loss_and_cd_t_together(D, dev):
    """The gd1 / gd2 path of the backward: cd_t's gradient arrives as dist1 / dist2 gradients."""
    x, gt = R.make_inputs(24, 3, 257, 1025)
    _run_case(D, dev, x, gt, 200, 0.5, False, {"loss": R.cotangent(3), "cd_t": R.cotangent(3, 2.0)}, "loss + cd_t")


def test_distances_alone(D, dev):
    """No gradient through the loss (a None upstream gradient passes NULL), different on each side."""
    x, gt = R.make_inputs(25, 2, 300, 200)
    r = np.random.default_rng(25)
    _run_case(D, dev, x, gt, 200, 1, False, {"dist1": r.standard_normal((2, 200))}, "dist1 alone")
    _run_case(D, dev, x, gt, 200, 1, False, {"dist1": r.standard_normal((2, 200)), "dist2": r.standard_normal((2, 300))},
              "dist1 + dist2")


@pytest.mark.parametrize("wrt", [("x",), ("gt",)])
def test_one_side_requires_grad(D, dev, wrt):
    x, gt = R.make_inputs(26, 2, 300, 1100)
    _run_case(D, dev, x, gt, 200, 0.5, False, {"loss": R.cotangent(2), "cd_t": R.cotangent(2)}, f"only {wrt[0]}", wrt=wrt)


# ---------------- routing ----------------

def test_calc_dcd_under_autograd_is_the_function(D, dev):
    from chamfer3D.model_utils import calc_dcd
    x, gt = R.make_inputs(30, 2, 300, 200)
    xg, gg = _t(x).to(dev).requires_grad_(True), _t(gt).to(dev)
    res = calc_dcd(xg, gg, alpha=200, n_lambda=0.5, return_raw=True)
    res[0].sum().backward()
    g_route = xg.grad.clone()
    assert type(res[0].grad_fn).__name__.startswith("DcdLossFn")
    xg.grad = None
    loss, d1, d2, i1, i2 = D.dcd_loss(xg, gg, alpha=200, n_lambda=0.5)
    loss.sum().backward()
    assert torch.equal(res[0], loss) and torch.equal(res[3], d1) and torch.equal(res[4], d2)
    assert torch.equal(res[5], i1) and torch.equal(res[6], i2) and torch.equal(g_route, xg.grad)
    o = nn_ref.nn_fwd(gt, x)
    r64, _ = R.run(x, gt, o[2], o[3], 200, 0.5)
    for k, got in (("cd_p", res[1]), ("cd_t", res[2])):
        assert got.requires_grad
        assert (got.detach().double().cpu() - r64[k]).abs().max().item() <= TOL


def test_fractional_lambda_without_autograd(D, dev):
    """lambda = 0.5 (cfgs/pcn_dcd.yaml) on the forward-only path: a truncation to 0 is off by ~0.1."""
    from chamfer3D.model_utils import calc_dcd
    from ured_hip import nn as unn
    x, gt = R.make_inputs(31, 3, 300, 200)
    o = nn_ref.nn_fwd(gt, x)
    r64, _ = R.run(x, gt, o[2], o[3], 200, 0.5)
    xg, gg = _t(x).to(dev), _t(gt).to(dev)
    with torch.no_grad():
        res = calc_dcd(xg, gg, alpha=200, n_lambda=0.5)
    d1, d2, i1, i2 = unn.nn_dense(gg, xg)
    res2 = unn.dcd(d1, i1, d2, i2, 200, 0.5)
    for got in (res, res2):
        for k, v in zip(("loss", "cd_p", "cd_t"), got):
            err = (v.double().cpu() - r64[k]).abs().max().item()
            assert err <= TOL, f"{k}: {err:.3e} off float64"


@pytest.mark.parametrize("lam", [0, 1, 2, 3])
def test_integral_lambda_is_ured_dcd_bitwise(D, dev, lam):
    from ured_hip import _lib, nn as unn
    x, gt = R.make_inputs(32, 3, 300, 200)
    d1, d2, i1, i2 = unn.nn_dense(_t(gt).to(dev), _t(x).to(dev))
    got = unn.dcd(d1, i1, d2, i2, 200, lam)
    out = torch.empty(3, 3, device=dev)
    _lib.call("ured_dcd", _lib.ptr(d1), _lib.ptr(i1), _lib.ptr(d2), _lib.ptr(i2), 3, 200, 300, 200.0, lam,
              300 / 200, 200 / 300, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_of(d1))
    for a, b in zip(got, out):
        assert torch.equal(a, b)
    if lam < 3:      # the special-cased exponents of the float kernel give ured_dcd's bits too
        loss = D.dcd_loss(_t(x).to(dev), _t(gt).to(dev), alpha=200, n_lambda=lam)[0]
        assert torch.equal(loss, out[0])


def test_limit_is_refused(D, dev):
    from ured_hip import _lib
    x = torch.zeros(1, 8193, 3, device=dev, requires_grad=True)
    gt = torch.zeros(1, 8192, 3, device=dev)
    with pytest.raises(_lib.UredError, match="exceeds"):
        D.dcd_loss(x, gt)


def test_captures_into_a_graph(D, dev):
    """Caller's stream, no host synchronisation, no allocation inside the library: forward and
    backward replayed on new inputs equal the eager run. Single stream, no branches."""
    x, gt = R.make_inputs(33, 2, 300, 200)
    xg, gg = _t(x).to(dev).requires_grad_(True), _t(gt).to(dev).requires_grad_(True)

    def step():
        loss = D.dcd_loss(xg, gg, alpha=200, n_lambda=0.5)[0]
        return torch.autograd.grad(loss.sum(), (xg, gg))

    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    x2, gt2 = R.make_inputs(34, 2, 300, 200)
    with torch.no_grad():
        xg.copy_(_t(x2).to(dev))
        gg.copy_(_t(gt2).to(dev))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(step(), captured):
        assert torch.equal(a, b)
