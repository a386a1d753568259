"""The per-tensor tolerance of the kernel-level parity tests (the idiom of tests/test_chain_gpu.py):

    err(gpu, ref64) <= 3 * err(ref32, ref64) + f * max|ref64|

ref32 is the same restatement run in float32 on the CPU, f = F_FWD for forward values and F_GRAD for
gradients. Nothing is derived from the GPU's output. Every check prints err / tol and records the
worst ratio of its kernel family in the caller's `worst` dict."""
import torch

F_FWD, F_GRAD, FLOOR_MULT = 1e-5, 2e-5, 3.0


def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


def check(worst, family, what, got, r32, r64, f):
    got, r32, r64 = _d(got), _d(r32), _d(r64)
    assert got.shape == r64.shape == r32.shape, (family, what, got.shape, r32.shape, r64.shape)
    if got.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), f"{family} {what}: non-finite values"
    err = (got - r64).abs().max().item()
    tol = FLOOR_MULT * (r32 - r64).abs().max().item() + f * r64.abs().max().item()
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    if ratio >= worst.get(family, (-1.0, ""))[0]:
        worst[family] = (ratio, what)
    print(f"{family:18s} {what:60s} err {err:.3e} tol {tol:.3e} ratio {ratio:.3f}")
    assert err <= tol, f"{family} {what}: err {err:.3e} > 3 x fp32 floor + {f:.0e} x max = {tol:.3e}"
    return ratio
