"""tests/shape_ref.py (the float64 reference of tests/test_shape_gpu.py) pinned without a GPU: equal,
part by part, to dataset.dataset_utils.get_shape_numpy (the reference's numpy form, dataset_utils.py:
601-621) to 1e-12, its autograd gradient equal to finite differences (torch.autograd.gradcheck) and
to the closed form weight * C^T A^T g."""
import numpy as np
import pytest
import torch

import shape_ref as R

F64 = torch.float64


def _case(J, n, seed, S=None):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    return dict(A=r(S or J, 3 * n, 6), param=r(J, 6), default=r(J, 6), init=r(6), conn=r(J, 6, 6), go=r(J, 3 * n))


@pytest.mark.parametrize("with_default", [True, False])
@pytest.mark.parametrize("with_conn", [True, False])
@pytest.mark.parametrize("with_init", [True, False])
def test_float64_equals_get_shape_numpy(with_default, with_conn, with_init):
    from dataset.dataset_utils import get_shape_numpy
    J, n, w = 5, 7, 0.3
    c = _case(J, n, 11)
    dflt, conn, init = (c["default"] if with_default else None, c["conn"] if with_conn else None,
                        c["init"] if with_init else None)
    out = R.get_shape(c["A"], c["param"], dflt, w, init, conn)
    assert out.shape == (J, 3 * n) and out.dtype == F64
    for j in range(J):
        prm = c["param"][j].numpy() - (init.numpy() if with_init else 0.0)
        want = get_shape_numpy(c["A"][j].numpy(), prm, None if dflt is None else dflt[j].numpy(), w,
                               None if conn is None else conn[j].numpy())
        assert want.shape == (n, 3)
        assert np.abs(out[j].reshape(n, 3).numpy() - want).max() <= 1e-12, j


def test_src_float64_equals_get_shape_numpy():
    from dataset.dataset_utils import get_shape_numpy
    S, n, w = 7, 5, 0.3
    labels = torch.tensor([-7, 6, -1, 0, 3, 3])
    c = _case(labels.numel(), n, 12, S=S)
    out = R.get_shape_src(c["A"], labels, c["param"], c["default"], w)
    mats = c["A"].numpy()
    for j, lab in enumerate(labels.tolist()):
        want = get_shape_numpy(mats[lab], c["param"][j].numpy(), c["default"][j].numpy(), w)   # python indexing
        assert np.abs(out[j].reshape(n, 3).numpy() - want).max() <= 1e-12, j
    assert torch.equal(out[0], R.get_shape(c["A"][0:1], c["param"][0:1], c["default"][0:1], w)[0])     # -S is row 0
    assert torch.equal(out[4], R.get_shape(c["A"][3:4], c["param"][4:5], c["default"][4:5], w)[0])


def test_gradcheck():
    c = _case(3, 4, 13)
    p = c["param"].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q: R.get_shape(c["A"], q, c["default"], 0.3, c["init"], c["conn"]), (p,))
    assert torch.autograd.gradcheck(lambda q: R.get_shape(c["A"], q), (p,))
    m = _case(3, 4, 14, S=7)
    labels = torch.tensor([-7, 6, 2])
    assert torch.autograd.gradcheck(lambda q: R.get_shape_src(m["A"], labels, q, m["default"], 0.3), (p,))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_run_gradient_closed_form(dtype):
    """run(): the gradient of param is weight * C^T (A^T g) per part slot, in param's own shape."""
    J, n, w = 6, 5, 0.3
    c = _case(J, n, 15)
    prm = c["param"].view(2, 3, 6)
    out, gp = R.run(dtype, c["A"], prm, c["go"], c["default"], w, c["init"], c["conn"])
    assert out.dtype == dtype and gp.dtype == dtype and gp.shape == prm.shape
    want = w * torch.bmm(c["conn"].transpose(1, 2), torch.bmm(c["A"].transpose(1, 2), c["go"].unsqueeze(-1))).squeeze(-1)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert (gp.double().view(J, 6) - want).abs().max().item() <= tol * want.abs().max().item()
    out2, none = R.run(dtype, c["A"], prm)
    assert none is None and out2.shape == (J, 3 * n)
    lab = torch.tensor([[-6, 5, 0], [2, 2, 2]])
    out3, gp3 = R.run(dtype, c["A"], prm, c["go"], c["default"], w, labels=lab)
    want3 = w * torch.bmm(c["A"][lab.reshape(-1)].transpose(1, 2), c["go"].unsqueeze(-1)).squeeze(-1)
    assert (gp3.double().view(J, 6) - want3).abs().max().item() <= tol * want3.abs().max().item()
