"""get_shape on the GPU (csrc/nn.hip: ured_get_shape_fwd/bwd, ured_get_shape_src_fwd/bwd, behind
ured_hip.ops.GetShapeFn / GetShapeSrcFn and dataset.dataset_utils.get_shape / get_shape_src) against
tests/shape_ref.py, which tests/test_shape_ref.py pins to the reference's numpy form and to finite
differences.

Tolerance, from tests/tol_check.py: err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|, f = 1e-5
for values and 2e-5 for gradients; ref32 is the same restatement in float32 on the CPU. Nothing is
derived from the GPU's output. Every gradient of two runs is compared bit for bit.

Row counts: the forward runs one thread per output row in blocks of 256 (a partially filled last block
unless J * R is a multiple of 256), the backward one block per part slot whose 256 threads stride over
the R rows (R < 64: waves without a row; R % 256 != 0: a tail trip; R = 0: nothing to sum)."""
import numpy as np
import pytest
import torch

import shape_ref as SR
from tol_check import F_FWD, F_GRAD, check

pytestmark = pytest.mark.gpu
WORST = {}
F32, F64 = torch.float32, torch.float64
ROWS = [1, 3, 63, 64, 65, 255, 256, 257, 771, 3075]
S_SRC = 7
SRC_LABELS = {1: [-S_SRC], 5: [-S_SRC, S_SRC - 1, -1, 3, 3]}


@pytest.fixture(scope="module")
def ops(dev):
    from ured_hip import ops
    yield ops
    for fam, (ratio, what) in sorted(WORST.items()):
        print(f"worst ratio {fam:18s} {ratio:.3f}  ({what})")


def _randn(g, *s):
    return torch.randn(*s, generator=g)


def _twice(fn, prm, go, dev):
    """fn(param on the device) -> out, run twice from fresh leaves: (out, grad) of each run."""
    runs = []
    for _ in range(2):
        p = prm.clone().to(dev).requires_grad_(True)
        out = fn(p)
        out.backward(go.to(dev).reshape(out.shape))
        runs.append((out.detach(), p.grad))
    assert torch.equal(runs[0][0], runs[1][0]), "values differ between two runs"
    assert torch.equal(runs[0][1], runs[1][1]), "gradients differ between two runs"
    return runs[0]


def _check(fam, tag, got, ref_kw, A, prm, go):
    o64, g64 = SR.run(F64, A, prm, go, **ref_kw)
    o32, g32 = SR.run(F32, A, prm, go, **ref_kw)
    check(WORST, fam + " fwd", tag, got[0].reshape(o64.shape), o32, o64, F_FWD)
    check(WORST, fam + " grad", tag, got[1], g32, g64, F_GRAD)


def _direct(ops, dev, J, R, seed):
    g = torch.Generator().manual_seed(seed)
    A, p, go = _randn(g, J, R, 6), _randn(g, J, 6), _randn(g, J, R)
    Ad = A.to(dev)
    _check("get_shape", f"J{J} R{R}", _twice(lambda q: ops.GetShapeFn.apply(Ad, q), p, go, dev), {}, A, p, go)
    return g


def _direct_src(ops, dev, labels, R, g, weight=0.3, with_dflt=True):
    J = len(labels)
    mats, p, go = _randn(g, S_SRC, R, 6), _randn(g, J, 6), _randn(g, J, R)
    dflt = _randn(g, J, 6) if with_dflt else None
    lab = torch.tensor(labels, dtype=torch.int64)
    md, ld, dd = mats.to(dev), lab.to(dev), None if dflt is None else dflt.to(dev)
    got = _twice(lambda q: ops.GetShapeSrcFn.apply(md, ld, q, dd, weight), p, go, dev)
    _check("get_shape_src", f"J{J} R{R} w{weight} dflt{int(with_dflt)}", got,
           dict(default=dflt, weight=weight, labels=lab), mats, p, go)


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("J", [1, 5])
def test_get_shape_rows_vs_float64(ops, dev, J, R):
    g = _direct(ops, dev, J, R, 1000 * J + R)
    _direct_src(ops, dev, SRC_LABELS[J], R, g)


def test_get_shape_bwd_zero_rows(dev):
    """R = 0 (the backward alone; the forward returns before its launch): every block finds no row and
    writes the zero gradient over whatever the buffer held."""
    from ured_hip import _lib
    J = 5
    g = torch.Generator().manual_seed(5)
    A, go = _randn(g, S_SRC, 1, 6).to(dev), _randn(g, J, 1).to(dev)      # valid pointers; no row is read
    lab = torch.tensor(SRC_LABELS[J], dtype=torch.int64, device=dev)
    gp = torch.full((J, 6), float("nan"), device=dev)
    _lib.call("ured_get_shape_bwd", _lib.ptr(A), _lib.ptr(go), J, 0, _lib.ptr(gp), _lib.stream_of(A))
    assert bool((gp == 0).all())
    gp.fill_(float("nan"))
    _lib.call("ured_get_shape_src_bwd", _lib.ptr(A), _lib.ptr(lab), S_SRC, _lib.ptr(go), 0.3, J, 0, _lib.ptr(gp),
              _lib.stream_of(A))
    assert bool((gp == 0).all())


# every slot of sample 1 reads the same source; -S and S - 1 are the extremes of python indexing
LABELS_BP = [[-S_SRC, S_SRC - 1, -1, 0], [2, 2, 2, 2], [-3, 5, -S_SRC, S_SRC - 1]]


@pytest.mark.parametrize("with_dflt", [True, False])
@pytest.mark.parametrize("weight", [0.3, 1.0])
def test_get_shape_src_labels_vs_float64(ops, dev, weight, with_dflt):
    """dataset_utils.get_shape_src over a SourceDB of S = 7 sources, [B, P] labels."""
    from dataset.dataset_utils import get_shape_src
    from train_utils.load_sources import SourceDB
    g = torch.Generator().manual_seed(21)
    n, (B, P) = 257, (len(LABELS_BP), len(LABELS_BP[0]))
    mats = _randn(g, S_SRC, 3 * n, 6)
    db = SourceDB(_randn(g, S_SRC, n, 3), mats, _randn(g, S_SRC, 6), torch.zeros(S_SRC, dtype=torch.int64), dev)
    lab = torch.tensor(LABELS_BP, dtype=torch.int64)
    prm, go = _randn(g, B, P, 6), _randn(g, B, P, n, 3)
    dflt = _randn(g, B, P, 6) if with_dflt else None
    dd = None if dflt is None else dflt.to(dev)

    def fn(q):
        out = get_shape_src(db, lab.to(dev), q, dd, weight)
        assert out.shape == (B, P, n, 3)
        return out
    got = _twice(fn, prm, go, dev)
    _check("get_shape_src", f"labels [B,P] w{weight} dflt{int(with_dflt)}", got,
           dict(default=dflt, weight=weight, labels=lab), mats, prm, go)
    assert got[1].shape == prm.shape


@pytest.mark.parametrize("branch", ["param_init", "connectivity_mat"])
def test_get_shape_wrapper_branches_vs_float64(ops, dev, branch):
    """dataset_utils.get_shape with param_init (a shared [6] offset subtracted before the weight) and
    with connectivity_mat ([B * P, 6, 6], applied to the finished parameters): the same kernels behind
    a few torch ops; values and the gradient that reaches `param`."""
    from dataset.dataset_utils import get_shape
    g = torch.Generator().manual_seed(22)
    B, P, n, w = 2, 3, 257, 0.3
    A, prm, dflt, go = _randn(g, B, P, 3 * n, 6), _randn(g, B, P, 6), _randn(g, B, P, 6), _randn(g, B, P, n, 3)
    init = _randn(g, 6) if branch == "param_init" else None
    conn = _randn(g, B * P, 6, 6) if branch == "connectivity_mat" else None
    Ad, dd = A.to(dev), dflt.to(dev)
    kw = dict(param_init=None if init is None else init.to(dev),
              connectivity_mat=None if conn is None else conn.to(dev))
    got = _twice(lambda q: get_shape(Ad, q, dd, w, **kw), prm, go, dev)
    assert got[0].shape == (B, P, n, 3)
    _check("get_shape wrapper", branch, got, dict(default=dflt, weight=w, param_init=init, connectivity_mat=conn),
           A.view(B * P, 3 * n, 6), prm, go)


def _sweep():
    rng = np.random.Generator(np.random.PCG64(20240607))
    return [(int(rng.integers(1, 41)), int(rng.integers(1, 1101))) for _ in range(32)]


@pytest.mark.parametrize("J,R", _sweep())
def test_get_shape_seeded_sweep(ops, dev, J, R):
    g = _direct(ops, dev, J, R, 7 * J + R)
    labels = torch.randint(-S_SRC, S_SRC, (J,), generator=g).tolist()
    _direct_src(ops, dev, labels, R, g, weight=1.0 if R % 2 else 0.3, with_dflt=bool(J % 2))
