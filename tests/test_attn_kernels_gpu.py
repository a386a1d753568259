"""csrc/attn.hip (ured_attn_fwd / ured_attn_bwd and the multi-set launches) held to the float64
restatement tests/node_ref.py::attn_fwd / attn_bwd (pinned on the CPU by tests/test_node_ref.py to
autograd through the reference's softmax_attention), through cross_attention, self_attention,
self_attention_pair and through direct calls where a stride or an address must differ:

  shapes     n = 1, m = 1 (weights exactly 1, dq and dk exactly 0), d = 1, 32 nodes, B in {1, 3};
  load path  the 16-byte loads need d, the row stride and the head offset h * d to be multiples of 4
             and a 16-byte aligned address; an odd row stride, an address one float off and a d that
             is no multiple of 4 (the head offset cannot break on its own: it is h * d) put the 4-byte
             path to work, on the same values and with the same bits;
  strides    every row stride larger than H * d, sentinels in the padding that must survive;
  logits     q and k scaled by 6 and 12 (|logit| to ~500, far past exp's fp32 range without the
             max subtraction), a row of equal logits (uniform weights, exactly), a row with one
             logit 200 above the rest (one-hot, exactly: the others underflow to 0);
  weights    the saved softmax weights against float64, their rows summing to 1 within m * 2^-23;
  maxima     forward and backward at the declared maxima n = m = 32, d = 128 (the backward needs
             74,240 B of LDS, above the 64 KB default) and around the old 64 KB boundary;
  sets       one cross-shaped and one self-shaped set of different n, m, d, H in one launch, and a
             launch with a B = 0 set, bitwise the single launches.

Tolerance: tests/tol_check.py (3 x the float32 restatement's own error + 1e-5 forward / 2e-5
gradients of the largest float64 element), per tensor. A second run of every case is bitwise the
first."""
import ctypes

import pytest
import torch

import node_ref as NR
from step_parity import report
from tol_check import F_FWD, F_GRAD, check

pytestmark = pytest.mark.gpu

SENT = -777.25
WORST = {}
NAMES = ("out", "w", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def hip(dev):
    from ured_hip import _lib, attn
    return attn, _lib


def _data(B, H, n, m, d, seed, mul=1.0):
    g = torch.Generator().manual_seed(seed)
    C = H * d
    return (torch.randn(B, n, C, generator=g) * mul, torch.randn(B, m, C, generator=g) * mul,
            torch.randn(B, m, C, generator=g), torch.randn(B, n, C, generator=g))


def ref_all(q, k, v, go, H, dt):
    scale = (q.shape[-1] // H) ** -0.5
    out, P = NR.attn_fwd(q, k, v, H, scale, dt)
    return (out, P) + NR.attn_bwd(q, k, v, P, go, H, scale, dt)


def run_cross(attn, dev, q, k, v, go, H):
    """cross_attention on q and the fused k|v -> (out, saved weights, dq, dk, dv)."""
    C = q.shape[-1]
    qd = q.to(dev).requires_grad_(True)
    kvd = torch.cat([k, v], -1).to(dev).requires_grad_(True)
    out = attn.cross_attention(qd, kvd, H)
    w = out.grad_fn.saved_tensors[2]
    out.backward(go.to(dev))
    return out.detach(), w, qd.grad, kvd.grad[..., :C], kvd.grad[..., C:]


def run_self(attn, dev, q, k, v, go, H):
    C = q.shape[-1]
    x = torch.cat([q, k, v], -1).to(dev).requires_grad_(True)
    out = attn.self_attention(x, H)
    w = out.grad_fn.saved_tensors[1]
    out.backward(go.to(dev))
    return out.detach(), w, x.grad[..., :C], x.grad[..., C:2 * C], x.grad[..., 2 * C:]


def compare(what, got, q, k, v, go, H):
    r32, r64 = ref_all(q, k, v, go, H, torch.float32), ref_all(q, k, v, go, H, torch.float64)
    for name, g, a, b in zip(NAMES, got, r32, r64):
        grad = name.startswith("d")
        check(WORST, "attention bwd" if grad else "attention fwd", f"{what} {name}", g, a, b, F_GRAD if grad else F_FWD)
    w, m = got[1].double().cpu(), k.shape[1]
    assert (w.sum(-1) - 1).abs().max().item() <= m * 2.0 ** -23, f"{what}: weight rows do not sum to 1"
    assert bool((w >= 0).all())


def same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), f"{what}: {name} differs"


SHAPES = [(1, 1, 1, 1), (1, 7, 5, 3), (7, 1, 5, 3), (32, 1, 8, 2), (1, 32, 8, 2), (32, 32, 8, 1), (5, 7, 16, 2)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n,m,d,H", SHAPES)
def test_cross_attention_shapes(dev, hip, n, m, d, H, B):
    attn, _ = hip
    q, k, v, go = _data(B, H, n, m, d, 100 * n + 10 * m + d + B)
    got = run_cross(attn, dev, q, k, v, go, H)
    same(got, run_cross(attn, dev, q, k, v, go, H), "two runs")
    compare(f"cross B{B} n{n} m{m} d{d} H{H}", got, q, k, v, go, H)
    if m == 1:          # one key: the weight is exp(0) / exp(0), and dS = P * (dP - P * dP) * scale = 0
        assert torch.equal(got[1], torch.ones_like(got[1]))
        assert torch.equal(got[2], torch.zeros_like(got[2])) and torch.equal(got[3], torch.zeros_like(got[3]))
        assert torch.equal(got[0], v.to(dev).expand(B, n, H * d))
    if n == m:          # the same problem through the fused q|k|v entry
        same(got, run_self(attn, dev, q, k, v, go, H), "self_attention vs cross_attention")


@pytest.mark.parametrize("B,H,n0,n1,d", [(3, 3, 1, 7, 5), (1, 1, 32, 1, 1), (2, 2, 5, 32, 8)])
def test_self_attention_pair_shapes(dev, hip, B, H, n0, n1, d):
    """The two-set launch of a self-attention layer against float64, set by set."""
    attn, _ = hip
    C = H * d
    sets = [_data(B, H, n, n, d, 7 * n + d) for n in (n0, n1)]
    x = torch.cat([torch.cat(s[:3], -1).reshape(-1, 3 * C) for s in sets]).to(dev).requires_grad_(True)
    go = torch.cat([s[3].reshape(-1, C) for s in sets]).to(dev)
    out = attn.self_attention_pair(x, B, n0, n1, H)
    w0 = out.grad_fn.saved_tensors[1]
    out.backward(go)
    r0, wo = 0, 0
    for n, (q, k, v, g) in zip((n0, n1), sets):
        rows = slice(r0, r0 + B * n)
        gx = x.grad[rows].view(B, n, 3 * C)
        got = (out.detach()[rows].view(B, n, C), w0[wo:wo + B * H * n * n].view(B, H, n, n), gx[..., :C], gx[..., C:2 * C],
               gx[..., 2 * C:])
        compare(f"pair B{B} H{H} n{n} d{d}", got, q, k, v, g, H)
        same(got, run_self(attn, dev, q, k, v, g, H), "pair vs single")
        r0, wo = r0 + B * n, wo + B * H * n * n


# ---- direct calls: strides, addresses, load paths -------------------------------------------------

class Region:
    """A [rows, C] matrix with row stride ld starting `off` floats into a flat buffer (NaN padding
    for an input, the sentinel for an output)."""

    def __init__(self, dev, rows, C, ld, off, vals=None):
        self.buf = torch.full((rows * ld + off + 8,), float("nan") if vals is not None else SENT, device=dev)
        self.view = self.buf.as_strided((rows, C), (ld, 1), off)
        if vals is not None:
            self.view.copy_(vals.reshape(rows, C).to(dev))
        self.ld, self.addr = ld, self.buf.data_ptr() + 4 * off

    def result(self, shape, what):
        got = self.view.clone().view(shape)
        self.view.fill_(SENT)
        assert bool((self.buf == SENT).all()), f"{what}: wrote outside its rows' H * d columns"
        return got


def direct(lib, dev, q, k, v, go, H, lay):
    """ured_attn_fwd + ured_attn_bwd with every tensor in its own buffer; lay[name] = (row stride,
    offset of the first element in floats) for q, k, v, out, dout, dq, dk, dv."""
    B, n, C = q.shape
    m, d = k.shape[1], C // H
    scale = float(d) ** -0.5
    R = {nm: Region(dev, B * r, C, *lay[nm], vals=t) for nm, t, r in (("q", q, n), ("k", k, m), ("v", v, m), ("dout", go, n))}
    R.update({nm: Region(dev, B * r, C, *lay[nm]) for nm, r in (("out", n), ("dq", n), ("dk", m), ("dv", m))})
    w = torch.full((B * H * n * m + 3,), SENT, device=dev)
    st = lib.current_stream()
    lib.call("ured_attn_fwd", R["q"].addr, R["q"].ld, R["k"].addr, R["k"].ld, R["v"].addr, R["v"].ld, B, H, n, m, d,
             scale, R["out"].addr, R["out"].ld, w.data_ptr(), st)
    lib.call("ured_attn_bwd", R["q"].addr, R["q"].ld, R["k"].addr, R["k"].ld, R["v"].addr, R["v"].ld, w.data_ptr(),
             R["dout"].addr, R["dout"].ld, B, H, n, m, d, scale, R["dq"].addr, R["dq"].ld, R["dk"].addr, R["dk"].ld,
             R["dv"].addr, R["dv"].ld, st)
    assert bool((w[B * H * n * m:] == SENT).all())
    return (R["out"].result((B, n, C), "out"), w[:B * H * n * m].view(B, H, n, m).clone(), R["dq"].result((B, n, C), "dq"),
            R["dk"].result((B, m, C), "dk"), R["dv"].result((B, m, C), "dv"))


TENSORS = ("q", "k", "v", "out", "dout", "dq", "dk", "dv")


def test_load_paths_same_bits(dev, hip):
    """d = 8, H = 2: tight aligned rows take the 16-byte loads. An odd row stride or an address one
    float off takes each input (q, k, v, dout), alone and all together, to the 4-byte loads; the
    output strides vary along. Same values, same bits, and the padding survives."""
    _, lib = hip
    B, H, n, m, d = 3, 2, 5, 7, 8
    C = H * d
    q, k, v, go = _data(B, H, n, m, d, 5)
    base = direct(lib, dev, q, k, v, go, H, {t: (C, 0) for t in TENSORS})
    same(base, direct(lib, dev, q, k, v, go, H, {t: (C, 0) for t in TENSORS}), "two runs")
    compare("direct aligned d8", base, q, k, v, go, H)
    padded = {t: (C + 4, 4) for t in TENSORS}              # still 16-byte aligned rows
    same(base, direct(lib, dev, q, k, v, go, H, padded), "padded aligned rows")
    for how, bad in (("odd row stride", (C + 5, 0)), ("address one float off", (C + 4, 1)), ("both", (C + 3, 3))):
        same(base, direct(lib, dev, q, k, v, go, H, {t: bad for t in TENSORS}), how)
        for t in ("q", "k", "v", "dout"):
            same(base, direct(lib, dev, q, k, v, go, H, dict(padded, **{t: bad})), f"{how}: {t} only")


@pytest.mark.parametrize("d,H", [(6, 1), (6, 2), (5, 3), (1, 4)])
def test_head_dim_not_a_multiple_of_four(dev, hip, d, H):
    """d % 4 != 0 (with H > 1 the head offsets h * d are unaligned as well): always the 4-byte loads,
    whatever the strides and addresses; the same bits in every placement, and float64."""
    _, lib = hip
    B, n, m = 2, 5, 7
    C = H * d
    q, k, v, go = _data(B, H, n, m, d, 11 + d)
    base = direct(lib, dev, q, k, v, go, H, {t: (C, 0) for t in TENSORS})
    compare(f"direct d{d} H{H}", base, q, k, v, go, H)
    for i, lay in enumerate(({t: ((C + 7) // 4 * 4, 0) for t in TENSORS}, {t: (C + 3, 1) for t in TENSORS},
                             {t: (C + 1 + j, j) for j, t in enumerate(TENSORS)})):
        same(base, direct(lib, dev, q, k, v, go, H, lay), f"placement {i}")


def test_row_strides_exceed_width(dev, hip):
    """Every stride different and larger than H * d, the fused layouts' case (q a column slice of
    [B, n, 3C]) taken further; against float64 and the tight run, padding intact (direct())."""
    _, lib = hip
    B, H, n, m, d = 2, 3, 9, 4, 12
    C = H * d
    q, k, v, go = _data(B, H, n, m, d, 23)
    lay = {t: (C + 4 * (j + 1), 4 * (j % 3)) for j, t in enumerate(TENSORS)}
    got = direct(lib, dev, q, k, v, go, H, lay)
    compare("direct strides", got, q, k, v, go, H)
    same(got, direct(lib, dev, q, k, v, go, H, {t: (C, 0) for t in TENSORS}), "tight rows")
    same(got, direct(lib, dev, q, k, v, go, H, {t: (3 * C + 1, 2) for t in TENSORS}), "wide odd rows")


# ---- the softmax ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mul", [1.0, 6.0, 12.0])
def test_large_logits(dev, hip, mul):
    """q and k scaled by 6 and 12: max |logit| ~ 160 and ~ 510 with a spread within one row up to
    ~ 780, where exp overflows fp32 without the row-max subtraction. Finite (tol_check) and within
    the tolerance of float64."""
    attn, _ = hip
    B, H, n, m, d = 2, 2, 5, 7, 16
    q, k, v, go = _data(B, H, n, m, d, 77, mul)
    S = torch.einsum("bihd,bjhd->bhij", q.double().view(B, n, H, d), k.double().view(B, m, H, d)) * d ** -0.5
    spread = (S.amax(-1) - S.amin(-1)).max().item()
    print(f"mul {mul}: max |logit| {S.abs().max().item():.1f}, largest spread within a row {spread:.1f}")
    if mul > 1:
        assert S.abs().max().item() > 88.8 and spread > 104     # past exp's fp32 overflow / underflow
    got = run_cross(attn, dev, q, k, v, go, H)
    same(got, run_cross(attn, dev, q, k, v, go, H), "two runs")
    compare(f"logits x{mul:g}", got, q, k, v, go, H)


def test_uniform_and_one_hot_rows(dev, hip):
    """Row 0: q = 0, so every logit is equal: weights exactly fp32(1 / m). Row 1: one logit 200
    above the rest: exp(-200) underflows, the row is exactly one-hot and passes no gradient to q and
    k. Row 2: random."""
    attn, _ = hip
    B, H, n, m, d = 1, 1, 3, 7, 16
    q, k, v, go = _data(B, H, n, m, d, 3)
    q[0, 0] = 0.0
    q[0, 1] = 0.0
    q[0, 1, 0] = 20.0                     # 20 * 40 * d^-0.5 = 200
    k[0, :, 0] = 0.0
    k[0, 0, 0] = 40.0
    got = run_cross(attn, dev, q, k, v, go, H)
    same(got, run_cross(attn, dev, q, k, v, go, H), "two runs")
    compare("uniform / one-hot", got, q, k, v, go, H)
    w = got[1][0, 0].cpu()
    assert torch.equal(w[0], (torch.ones(m) / torch.tensor(float(m))).float())
    assert torch.equal(w[1], torch.eye(m)[0])
    assert torch.equal(got[0][0, 1].cpu(), v[0, 0])
    assert torch.equal(got[2][0, 1].cpu(), torch.zeros(H * d))


# ---- the declared maxima ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,d", [(32, 32, 128), (29, 29, 128), (32, 32, 112), (28, 28, 128), (32, 1, 128), (1, 32, 128)])
def test_declared_maxima_forward_and_backward(dev, hip, n, m, d):
    """Every shape the forward accepts runs backward too. The backward's LDS image is
    4 * ((2n + 2m)(d + 1) + 2nm) bytes: 74,240 at (32, 32, 128), 66,584 at (29, 29, 128) and 66,048 at
    (32, 32, 112), all above the 64 KB a launch may ask for by default (these raised "needs more than
    64 KB of LDS" from backward after a successful forward), 64,064 at (28, 28, 128)."""
    attn, _ = hip
    q, k, v, go = _data(1, 1, n, m, d, n + m + d)
    got = run_cross(attn, dev, q, k, v, go, 1)
    same(got, run_cross(attn, dev, q, k, v, go, 1), "two runs")
    compare(f"maxima n{n} m{m} d{d}", got, q, k, v, go, 1)


# ---- multi-set launches ----------------------------------------------------------------------------

def _set_entry(attn, x, dev_t, B, H, n, m, d):
    """Fill one UredAttnSet from device tensors {q, k, v, out, w, dout, dq, dk, dv: (tensor, column)}."""
    for nm in ("q", "k", "v", "out", "dout", "dq", "dk", "dv"):
        t, col = dev_t[nm]
        setattr(x, nm, t.data_ptr() + 4 * col if t.numel() else None)
        setattr(x, "ld" + ("o" if nm == "out" else "do" if nm == "dout" else nm), t.shape[-1])
    x.weights = dev_t["w"].data_ptr() if dev_t["w"].numel() else None
    x.B, x.H, x.n, x.m, x.d, x.scale = B, H, n, m, d, float(d) ** -0.5


def _alloc(dev, q, k, v, go, H, fused):
    """Device tensors of one set: cross-shaped (q apart, k|v fused) or self-shaped (q|k|v fused)."""
    B, n, C = q.shape
    m = k.shape[1]
    w = torch.full((B, H, n, m), SENT, device=dev)
    out, dout = torch.full((B, n, C), SENT, device=dev), go.to(dev)
    if fused:
        x = torch.cat([q, k, v], -1).to(dev)
        gx = torch.full_like(x, SENT)
        return {"q": (x, 0), "k": (x, C), "v": (x, 2 * C), "out": (out, 0), "w": w, "dout": (dout, 0), "dq": (gx, 0),
                "dk": (gx, C), "dv": (gx, 2 * C)}
    qd, kv = q.to(dev), torch.cat([k, v], -1).to(dev)
    gq, gkv = torch.full_like(qd, SENT), torch.full_like(kv, SENT)
    return {"q": (qd, 0), "k": (kv, 0), "v": (kv, C), "out": (out, 0), "w": w, "dout": (dout, 0), "dq": (gq, 0),
            "dk": (gkv, 0), "dv": (gkv, C)}


def _results(T, C):
    return (T["out"][0].clone(), T["w"].clone(), T["dq"][0][..., T["dq"][1]:T["dq"][1] + C].clone(),
            T["dk"][0][..., T["dk"][1]:T["dk"][1] + C].clone(), T["dv"][0][..., T["dv"][1]:T["dv"][1] + C].clone())


def _launch_sets(attn, lib, dev, specs, together):
    """specs: [(data, H, fused)]; one two-set launch, or one launch per set -> per-set results."""
    Ts = [_alloc(dev, *data, H, fused) for data, H, fused in specs]
    arr = (attn.UredAttnSet * len(specs))()
    for x, T, (data, H, _) in zip(arr, Ts, specs):
        B, n, C = data[0].shape
        _set_entry(attn, x, T, B, H, n, data[1].shape[1], C // H)
    st = lib.current_stream()
    for name in ("ured_attn_fwd_sets", "ured_attn_bwd_sets"):
        if together:
            lib.call(name, len(specs), ctypes.byref(arr), st)
        else:
            for i in range(len(specs)):
                lib.call(name, 1, ctypes.byref(arr[i]), st)
    return [_results(T, data[0].shape[-1]) for T, (data, _, _) in zip(Ts, specs)]


def test_mixed_sets_equal_single_launches(dev, hip):
    """A cross-shaped set (n != m, q apart from the fused k|v) and a self-shaped set of another n, d
    and H in one forward and one backward launch: the LDS image is sized for the larger set and each
    block lays out its own. Bitwise the single launches, in either order, and float64."""
    attn, lib = hip
    cross = (_data(3, 2, 5, 7, 16, 1), 2, False)
    selfs = (_data(2, 3, 9, 9, 5, 2), 3, True)
    for specs in ([cross, selfs], [selfs, cross]):
        both = _launch_sets(attn, lib, dev, specs, True)
        again = _launch_sets(attn, lib, dev, specs, True)
        single = _launch_sets(attn, lib, dev, specs, False)
        for i, (data, H, fused) in enumerate(specs):
            same(both[i], again[i], "two runs")
            same(both[i], single[i], f"set {i} of a two-set launch vs its own launch")
            same(both[i], direct(lib, dev, *data, H, {t: (data[0].shape[-1], 0) for t in TENSORS}), "ured_attn_fwd / bwd")
            compare(f"sets {'self' if fused else 'cross'}", both[i], *data, H)


@pytest.mark.parametrize("empty_first", [True, False])
def test_launch_with_an_empty_set(dev, hip, empty_first):
    """A B = 0 set adds no workgroups (its pointers may be null); the other set's results are those
    of its own launch, and a launch of only empty sets does nothing."""
    attn, lib = hip
    real = (_data(2, 2, 5, 7, 16, 4), 2, False)
    empty = (_data(0, 3, 4, 4, 8, 5), 3, True)
    specs = [empty, real] if empty_first else [real, empty]
    both = _launch_sets(attn, lib, dev, specs, True)
    single = _launch_sets(attn, lib, dev, [real], False)
    same(both[1 if empty_first else 0], single[0], "beside an empty set")
    compare("beside an empty set", single[0], *real[0], 2)
    assert all(t.numel() == 0 for t in both[0 if empty_first else 1])
    _launch_sets(attn, lib, dev, [empty, empty], True)


def test_report_worst_ratios():
    """Not a check: the worst err / tolerance measured above, per kernel family."""
    for fam, (ratio, what) in sorted(WORST.items()):
        report(f"attention kernel parity, {fam}: worst err / tolerance {ratio:.3f} ({what})")
