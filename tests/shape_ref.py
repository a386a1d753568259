"""Plain torch restatement of get_shape (the reference's dataset/dataset_utils.py:691-726) for the
parity tests of ured_get_shape_fwd/bwd and ured_get_shape_src_fwd/bwd (csrc/nn.hip), runnable in
float64 and float32 on the CPU:

    p   = weight * (param - param_init) + default        [J, 6]
    p   = connectivity_mat @ p                           (optional, [J, 6, 6])
    out = A @ p                                          [J, R]

with the gradient of `param` by CPU autograd. get_shape_src is the same with A = mats[labels] (python
negative indexing, dataset_utils.py:800-805). tests/test_shape_ref.py pins the float64 form to
dataset.dataset_utils.get_shape_numpy and to finite differences."""
import torch


def _c(t, dtype):
    return None if t is None else torch.as_tensor(t).detach().cpu().to(dtype)


def params(param, default=None, weight=1.0, param_init=None, connectivity_mat=None):
    """[J, 6] parameters of the J part slots (param of any shape [..., 6])."""
    p = param.reshape(-1, 6)
    if param_init is not None:
        p = p - param_init.reshape(1, 6)
    p = weight * p
    if default is not None:
        p = p + default.reshape(-1, 6)
    if connectivity_mat is not None:
        p = torch.bmm(connectivity_mat, p.unsqueeze(-1)).squeeze(-1)
    return p


def get_shape(A, param, default=None, weight=1.0, param_init=None, connectivity_mat=None):
    """A [J, R, 6] -> out [J, R]."""
    p = params(param, default, weight, param_init, connectivity_mat)
    return torch.bmm(A, p.unsqueeze(-1)).squeeze(-1)


def get_shape_src(mats, labels, param, default=None, weight=1.0):
    """mats [S, R, 6], labels int64 [J] in [-S, S) -> out [J, R]."""
    return get_shape(mats[labels.reshape(-1)], param, default, weight)


def run(dtype, A, param, grad_out=None, default=None, weight=1.0, param_init=None, connectivity_mat=None,
        labels=None):
    """-> (out [J, R], grad of param in param's shape or None) in `dtype` on the CPU; with `labels`, A is
    the source database [S, R, 6]."""
    A, default, param_init, connectivity_mat = (_c(t, dtype) for t in (A, default, param_init, connectivity_mat))
    prm = _c(param, dtype).requires_grad_(grad_out is not None)
    if labels is not None:
        A = A[torch.as_tensor(labels).cpu().long().reshape(-1)]
    out = get_shape(A, prm, default, weight, param_init, connectivity_mat)
    if grad_out is None:
        return out.detach(), None
    out.backward(_c(grad_out, dtype).reshape(out.shape))
    return out.detach(), prm.grad
