"""The loss-head kernels (csrc/loss.hip) one entry point at a time against tests/loss_ref.py (float64;
pinned to the oracle by tests/test_loss_ref.py), at the sizes and inputs the head tests never reach:
several ranks' source codes (n_all > n, s_off > 0, ds == NULL), every strided loop with a second
trip (n, n_all, C, NP, N > 256), clamped norms, ignored rows up to all of them, exact zeros of the
L1 arguments, unused / masked source parts, U == 0, S > P*NP, the segment tables as such.
ured_hip.losshead is imported for the registered signatures and PointLossDesc only; the entries are
called through _lib.call with the test's own counter.

Every reducing entry (cd_pair_reduce, point_losses_fwd, contrast_fwd) is called on a counter that a
launch with another grid has used before, twice (bitwise equal), into NaN / -1 pre-filled outputs
(every element the header says is written must be), and must leave the counter at 0.

Tolerances
  * contrastive loss 2e-6 relative, its gradients 1e-5 of the tensor's largest entry (the head
    test's); rows with a clamped norm each against their own largest entry, the others against
    the others'. A comparison that does not fit is redone against the yardstick the project uses
    elsewhere: 3 x the error of the same loss composed of fp32 torch ops on the CPU, plus the floor.
    Measured (worst error / floor, MI355X): see the table at the end of this docstring.
  * inverse norms 2e-6 relative; lse within 2e-6 * scale (the logits lie in [-scale, scale] and lse
    inherits their absolute error).
  * fp32 sums of non-negative terms (cd_reduce, point-loss terms): (run + 8 + extra) * 2^-24 * sum,
    run = the per-thread additions of one block sum, 8 its tree levels, extra = the roundings
    outside it (the final fp32 store; for the source reconstruction the product with the slot
    weight). The point-loss inputs lie on the grid k/1024 in [-2, 2], so every L1 argument and
    every squared difference is exact in fp32 and signs agree with float64 everywhere.
  * per-distance weights: 4 * 2^-24 relative, elementwise (two products and a division).
  * prep, fold, assemble: bitwise.

Measured on MI355X (worst error / bound per entry point over all cases; contrast: error / floor):
  contrast_fwd  inv 0.064   lse 0.162   loss <= 1 but for the two C = 260 cases with t_i = s_i, where the
                loss is 1.7e-4 and all of it is log(1 + 1.7e-4) of an fp32 sum that holds a 1:
                (64,192,64,260) 43.8 (the fp32 torch composition: 17.3), (64,192,128,260) 123.6 (102.1);
                both pass on the 3 x yardstick. At n_all = 600 and C = 260 every other case fits the
                floor.
  contrast_bwd  dt 0.73   ds 0.77 (C = 260, t_i = +-s_i); no case needed the yardstick
  point_losses  terms 0.113   dres 0.004   drec 0.007   drecu 0.006
  cd_pair       reduce 0.117   grad 0.125 (of 4 * 2^-24); largest accepted 2B(P+1) = 8448 (the cap;
                163840 bytes of LDS per workgroup)
"""
import ctypes
import math

import pytest
import torch

import loss_ref
from loss_ref import U32, f64

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def H(dev):
    from ured_hip import losshead          # registers the entry points' signatures
    return losshead


def _call(name, *args):
    from ured_hip import _lib
    _lib.call(name, *args)


def _rejected(name, *args):
    from ured_hip import _lib
    with pytest.raises(_lib.UredError):
        _lib.call(name, *args)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    from ured_hip import _lib
    return _lib.stream_of(t)


def _note(name, err, bound):
    """Running worst error / bound of an entry point (printed: pytest -s shows it)."""
    r = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    if r > WORST.get(name, -1.0):
        WORST[name] = r
        print(f"{name}: worst error / bound so far {r:.3f}")
    return r


def _within(got, ref, bound, name):
    err = (f64(got) - f64(ref)).abs()
    over = err - f64(bound) * (1 + 1e-13) - 1e-300
    _note(name, (err / f64(bound).clamp_min(1e-300)).max().item(), 1.0)
    assert (over <= 0).all(), f"{name}: over the rounding bound by {over.max().item():.3e}"


def _counter(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _filled(dev, *shape, value=NAN, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=dev)


# ---------------------------------------------------------------------------------------------
# contrastive loss
# ---------------------------------------------------------------------------------------------
SCALE = float(torch.tensor(math.log(1 / 0.07), dtype=torch.float32).exp())
CONTRAST_CASES = [(5, 5, 0, 4), (300, 300, 0, 32), (64, 192, 64, 260), (64, 192, 128, 260), (300, 600, 300, 8)]
VARIANTS = ["plain", "some_ignored", "one_valid", "all_ignored", "zero_rows", "tiny_rows", "t_eq_s", "t_eq_minus_s"]


def _contrast_inputs(n, n_all, s_off, C, variant):
    g = torch.Generator().manual_seed(1000 * n + n_all + s_off + C)
    t = torch.randn(n, C, generator=g)
    s = torch.randn(n_all, C, generator=g)
    labels = torch.randint(0, 50, (n,), generator=g)
    own = []                                        # (t rows, s rows) with a clamped norm
    if variant == "some_ignored":
        labels[::7] = -1
        labels[1] = -1
    elif variant == "one_valid":
        labels[:] = -1
        labels[n // 2] = 3
    elif variant == "all_ignored":
        labels[:] = -1
    elif variant == "zero_rows":
        t[1] = 0
        s[s_off + 2] = 0
        own = [[1], [2]]
    elif variant == "tiny_rows":                    # norm about 1e-13 < 1e-12: clamped, yet not zero
        t[1] = torch.randn(C, generator=g) * (1e-13 / C ** 0.5)
        s[s_off + 2] = torch.randn(C, generator=g) * (1e-13 / C ** 0.5)
        own = [[1], [2]]
    elif variant == "t_eq_s":
        t = s[s_off:s_off + n].clone()
    elif variant == "t_eq_minus_s":
        t = -s[s_off:s_off + n]
    return t.contiguous(), s.contiguous(), labels, own


def _contrast_fwd(dev, t, s, labels, s_off, counter, loss_fill=NAN):
    n, C = t.shape
    n_all = s.shape[0]
    o = dict(inv=_filled(dev, n + n_all), lse=_filled(dev, n), ws=_filled(dev, 2 * n), loss=_filled(dev, 1, value=loss_fill))
    _call("ured_contrast_fwd", _p(t), _p(s), _p(labels), n, n_all, C, s_off, SCALE, _p(o["inv"]), _p(o["lse"]),
          _p(o["ws"]), _p(counter), _p(o["loss"]), _stream(t))
    assert counter.item() == 0, "the counter is not back at 0"
    return o


def _contrast_bwd(dev, t, s, labels, s_off, fwd, g, with_ds=True):
    n, C = t.shape
    dt = _filled(dev, n, C)
    ds = _filled(dev, n, C) if with_ds else None
    gd = torch.tensor([g], device=dev)
    _call("ured_contrast_bwd", _p(t), _p(s), _p(labels), n, s.shape[0], C, s_off, SCALE, _p(fwd["inv"]), _p(fwd["lse"]),
          _p(gd), _p(dt), _p(ds), _stream(t))
    return dt, ds


def _grad_check(name, got, ref, ref32, own):
    """Rows in `own` each against their own largest entry, the others together against theirs:
    within 1e-5 of it, else within 3 x the fp32 torch composition's error + that floor."""
    got, ref = f64(got), f64(ref)
    assert not torch.isnan(got).any(), f"{name}: unwritten or nan entries"
    rest = [r for r in range(ref.shape[0]) if r not in own]
    for rows in [[r] for r in own] + [rest]:
        if not rows:
            continue
        err = (got[rows] - ref[rows]).abs().max().item()
        floor = 1e-5 * ref[rows].abs().max().item()
        _note(name + " (error / floor)", err, floor)
        if err <= floor:
            continue
        err32 = (f64(ref32()[rows]) - ref[rows]).abs().max().item()
        print(f"{name} rows {rows[:3]}: error / floor {err / floor:.2f}, fp32 torch composition {err32 / floor:.2f}")
        assert err <= 3 * err32 + floor, f"{name} rows {rows[:3]}: {err:.3e} > 3 * {err32:.3e} + {floor:.3e}"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,n_all,s_off,C", CONTRAST_CASES)
def test_contrast(H, dev, n, n_all, s_off, C, variant):
    t, s, labels, own = _contrast_inputs(n, n_all, s_off, C, variant)
    td, sd, ld = t.to(dev), s.to(dev), labels.to(dev)
    counter = _counter(dev)
    # another grid on the same counter first (n = 3 rows), then the case, twice
    _contrast_fwd(dev, td[:3].contiguous(), sd, ld[:3].contiguous(), 0, counter)
    fill = 12345.0 if variant == "all_ignored" else NAN       # there nan is the answer
    f1 = _contrast_fwd(dev, td, sd, ld, s_off, counter, fill)
    f2 = _contrast_fwd(dev, td, sd, ld, s_off, counter, fill)
    for key in f1:
        assert torch.equal(f1[key].view(torch.int32), f2[key].view(torch.int32)), f"{key} differs between two calls"
    for key in ("inv", "lse", "ws"):
        assert not torch.isnan(f1[key]).any(), f"{key}: not every element written"
    ref = {g: loss_ref.contrast(t, s, labels, s_off, SCALE, g) for g in (1.0, -2.5)}
    r = ref[1.0]
    got = f1["loss"].item()
    valid = (labels != -1)
    assert torch.equal(f1["ws"].cpu()[1::2], valid.float())
    assert not f1["ws"].cpu()[0::2][~valid].any()
    if variant == "all_ignored":
        assert math.isnan(got) and math.isnan(r["loss"].item())
    else:
        err, floor = abs(got - r["loss"].item()), 2e-6 * abs(r["loss"].item())
        _note("contrast_fwd loss (error / floor)", err, floor)
        if err > floor:
            err32 = abs(loss_ref.contrast(t, s, labels, s_off, SCALE, dtype=torch.float32)["loss"].item() - r["loss"].item())
            print(f"contrast loss: error / floor {err / floor:.2f}, fp32 torch composition {err32 / floor:.2f}")
            assert err <= 3 * err32 + floor, f"loss {got} vs {r['loss'].item()}: {err:.3e} > 3 * {err32:.3e} + {floor:.3e}"
    _within(f1["inv"], r["inv"], 2e-6 * r["inv"], "contrast_fwd inv")
    _within(f1["lse"], r["lse"], torch.full((n,), 2e-6 * SCALE), "contrast_fwd lse")
    for g in (1.0, -2.5):
        dt, ds = _contrast_bwd(dev, td, sd, ld, s_off, f1, g)
        dt0, none = _contrast_bwd(dev, td, sd, ld, s_off, f1, g, with_ds=False)
        assert none is None and torch.equal(dt.view(torch.int32), dt0.view(torch.int32)), "dt depends on ds == NULL"
        if variant == "all_ignored":
            assert not dt.any() and not ds.any()
            continue
        r32 = {}

        def ref32(key, g=g):
            if not r32:
                r32.update(loss_ref.contrast(t, s, labels, s_off, SCALE, g, dtype=torch.float32))
            return r32[key]
        _grad_check("contrast_bwd dt", dt, ref[g]["dt"], lambda: ref32("dt"), own[0] if own else [])
        _grad_check("contrast_bwd ds", ds, ref[g]["ds"], lambda: ref32("ds"), own[1] if own else [])


def test_contrast_rejections(H, dev):
    """Host-side checks: UredError, and nothing is launched (outputs and counter untouched)."""
    n, C = 8, 8
    buf = torch.randn(4 * n * C + 4, device=dev)
    t, s = buf[:n * C].view(n, C), buf[n * C:4 * n * C].view(3 * n, C)
    labels = torch.zeros(n, dtype=torch.long, device=dev)
    counter = _counter(dev)
    out = dict(inv=_filled(dev, 4 * n), lse=_filled(dev, n), ws=_filled(dev, 2 * n), loss=_filled(dev, 1),
               dt=_filled(dev, n, C), ds=_filled(dev, n, C))
    g = torch.ones(1, device=dev)

    def fwd(t, s, n, n_all, C, s_off):
        _rejected("ured_contrast_fwd", _p(t), _p(s), _p(labels), n, n_all, C, s_off, SCALE, _p(out["inv"]), _p(out["lse"]),
                  _p(out["ws"]), _p(counter), _p(out["loss"]), _stream(buf))

    def bwd(t, s, n, n_all, C, s_off):
        _rejected("ured_contrast_bwd", _p(t), _p(s), _p(labels), n, n_all, C, s_off, SCALE, _p(out["inv"]), _p(out["lse"]),
                  _p(g), _p(out["dt"]), _p(out["ds"]), _stream(buf))

    t1 = buf[1:1 + n * C].view(n, C)                 # 4 bytes off a 16-byte boundary
    assert t.data_ptr() % 16 == 0 and t1.data_ptr() % 16 == 4
    for f in (fwd, bwd):
        f(t, s, n, n, 6, 0)                          # C % 4
        f(t1, s, n, n, C, 0)                         # misaligned t
        f(t, t1, n, n, C, 0)                         # misaligned s_all
        f(t, s, n, 4097, C, 0)                       # n_all > 4096
        f(t, s, n, 2 * n, C, n + 1)                  # s_off + n > n_all
        f(t, s, n, n, 1 << 22, 0)                    # 16 MB of LDS: beyond any device's workgroup limit
    torch.cuda.synchronize()
    assert counter.item() == 0
    for key, v in out.items():
        assert torch.isnan(v).all(), f"{key} was written by a rejected call"


# ---------------------------------------------------------------------------------------------
# residual + reconstruction losses
# ---------------------------------------------------------------------------------------------
POINT_CASES = [(1, 5, 3, 1, 1, 1), (2, 129, 40, 5, 342, 6), (3, 200, 64, 7, 64, 12), (2, 100, 16, 0, 8, 0)]
G4 = [1.5, -0.5, 2.0, -3.0]


def _grid(g, *shape):
    return torch.randint(-2048, 2049, shape, generator=g).float() / 1024


def _point_inputs(B, N, S, U, NP, R, mask_zero=False):
    g = torch.Generator().manual_seed(B * 1000 + N + U)
    x, out, rec = _grid(g, B, N, 3), _grid(g, B, S, 3), _grid(g, B, N, 3)
    res = _grid(g, B, N, 3)
    knn = torch.randint(0, S, (B, N), generator=g).int()
    knn[0, 0], knn[0, 1] = 0, S - 1
    nn = out[torch.arange(B).unsqueeze(1), knn.long()]
    e = torch.arange(B * N * 3).view(B, N, 3)
    z0, z1 = e % 4 == 0, e % 5 == 1                  # planted exact zeros of x + res - nn and of res
    res = torch.where(z0, nn - x, res)
    res = torch.where(z1 & ~z0, torch.zeros(()), res)
    d = dict(x=x, out=out, knn=knn, res=res, rec=rec, recu=None, ptsu=None, inv=None, mask=None, z0=z0, z1=z1 & ~z0)
    if U:
        d["recu"], d["ptsu"] = _grid(g, U, NP, 3), _grid(g, U, NP, 3)
        if U >= 3:      # part 1: three slots with masks 1, 0, 1; part U-1: no slot; the rest drawn
            inv = torch.randint(0, U - 1, (R,), generator=g)
            mask = torch.randint(0, 2, (R,), generator=g).float()
            inv[inv == 1] = 0
            inv[:3] = 1
            mask[:3] = torch.tensor([1.0, 0.0, 1.0])
        else:
            inv, mask = torch.zeros(R, dtype=torch.long), torch.ones(R)
        d["inv"], d["mask"] = inv, torch.zeros(R) if mask_zero else mask
    return d


def _point_desc(H, dev, d, dims):
    B, N, S, U, NP, R = dims
    dd = {k: (None if d[k] is None else d[k].to(dev).contiguous()) for k in ("x", "out", "knn", "res", "rec", "recu", "ptsu",
                                                                           "inv", "mask")}
    desc = H.PointLossDesc(B, N, S, U, NP, R, *[_p(dd[k]) for k in ("x", "out", "knn", "res", "rec", "recu", "ptsu",
                                                                   "inv", "mask")])
    return desc, dd


def _point_fwd(dev, desc, dims, counter, t3_fill=NAN):
    B, N, S, U, NP, R = dims
    ws = _filled(dev, 3 * ((B * N + 255) // 256 + U))
    terms = _filled(dev, 4)
    terms[3] = t3_fill
    _call("ured_point_losses_fwd", ctypes.byref(desc), _p(ws), _p(counter), _p(terms), _stream(ws))
    assert counter.item() == 0, "the counter is not back at 0"
    return ws, terms


def _point_bwd(dev, desc, dims):
    B, N, S, U, NP, R = dims
    dres, drec = _filled(dev, B, N, 3), _filled(dev, B, N, 3)
    drecu = _filled(dev, U, NP, 3) if U else None
    g4 = torch.tensor(G4, device=dev)
    _call("ured_point_losses_bwd", ctypes.byref(desc), _p(g4), _p(dres), _p(drec), _p(drecu), _stream(g4))
    return dres, drec, drecu


def _point_term_bounds(d, dims):
    """(run + 8 + extra) * 2^-24 * sum of the (exact, non-negative) terms, per loss term."""
    B, N, S, U, NP, R = dims
    x, res, rec = f64(d["x"]), f64(d["res"]), f64(d["rec"])
    nn = f64(d["out"])[torch.arange(B).unsqueeze(1), d["knn"].long()]
    M = B * N
    sums = [(x + res - nn).abs().sum() / M, res.abs().sum() / M, ((rec - x) ** 2).sum() / M]
    b = [(3 + 8 + 1) * U32 * v.item() for v in sums]       # one point (3 coordinates) per thread
    if U and d["mask"].sum() > 0:
        w = torch.zeros(U, dtype=torch.float64).index_add_(0, d["inv"], f64(d["mask"]))
        per = ((f64(d["recu"]) - f64(d["ptsu"])) ** 2).sum((1, 2))
        b.append((math.ceil(3 * NP / 256) + 8 + 2) * U32 * ((w * per).sum() / NP / f64(d["mask"]).sum()).item())
    return b


@pytest.mark.parametrize("B,N,S,U,NP,R", POINT_CASES)
def test_point_losses(H, dev, B, N, S, U, NP, R):
    dims = (B, N, S, U, NP, R)
    d = _point_inputs(*dims)
    # the grid makes the L1 arguments exact: fp32 and float64 agree bitwise, planted zeros included
    a32 = d["x"] + d["res"] - d["out"][torch.arange(B).unsqueeze(1), d["knn"].long()]
    a64 = f64(d["x"]) + f64(d["res"]) - f64(d["out"])[torch.arange(B).unsqueeze(1), d["knn"].long()]
    assert torch.equal(a32.double(), a64) and (a64[d["z0"]] == 0).all() and (f64(d["res"])[d["z1"]] == 0).all()
    assert d["z0"].float().mean() >= 0.2 and ((a64 == 0) | (d["res"] == 0)).float().mean() >= 0.3
    terms_ref, dres_ref, drec_ref, drecu_ref = loss_ref.point_losses(*[d[k] for k in ("x", "out", "knn", "res", "rec", "recu",
                                                                                       "ptsu", "inv", "mask")], G4)
    desc, keep = _point_desc(H, dev, d, dims)
    counter = _counter(dev)
    small = (1, 5, 3, 1, 1, 1)
    desc0, keep0 = _point_desc(H, dev, _point_inputs(*small), small)
    _point_fwd(dev, desc0, small, counter)                 # another grid on the same counter first
    fill = NAN if U else 12345.0                           # U == 0: nan is the answer
    ws, terms = _point_fwd(dev, desc, dims, counter, fill)
    ws2, terms2 = _point_fwd(dev, desc, dims, counter, fill)
    assert torch.equal(terms.view(torch.int32), terms2.view(torch.int32)) and torch.equal(ws.view(torch.int32),
                                                                                          ws2.view(torch.int32))
    assert not torch.isnan(ws).any(), "workspace: not every element written"
    bounds = _point_term_bounds(d, dims)
    _within(terms[:len(bounds)], terms_ref[:len(bounds)], torch.tensor(bounds), "point_losses_fwd terms")
    if U == 0:
        assert math.isnan(terms[3].item()) and math.isnan(terms_ref[3].item())
    dres, drec, drecu = _point_bwd(dev, desc, dims)
    for name, got, ref in (("dres", dres, dres_ref), ("drec", drec, drec_ref), ("drecu", drecu, drecu_ref)):
        if ref is None:
            assert got is None
            continue
        assert not torch.isnan(got).any(), f"{name}: not every element written"
        err = (f64(got) - ref).abs().max().item()
        tol = 1e-5 * ref.abs().max().item()
        _note("point_losses_bwd " + name, err, tol)
        assert err <= tol, f"{name}: {err:.3e} > {tol:.3e}"
    # the sign of every L1 argument, zeros included, none left out
    assert torch.equal(f64(dres) != 0, (a32 != 0) | (d["res"] != 0))       # |g0| != |g1|: no cancellation
    if U >= 3:
        assert not drecu[U - 1].any() and not drecu_ref[U - 1].any()          # the part no slot refers to
        assert drecu[1].any()


def test_point_losses_all_zero_mask(H, dev):
    """mask.sum() == 0: the weighted mean is 0/0; term 3 and drecu are nan as the reference's, the
    other terms and gradients are untouched by it. Every part is in some slot here: autograd leaves
    the rows of a part that no slot refers to at 0, the kernel writes nan there as well
    (include/ured_hip.h)."""
    dims = POINT_CASES[2]
    d = _point_inputs(*dims, mask_zero=True)
    d["inv"] = torch.arange(dims[5]) % dims[3]
    terms_ref, dres_ref, drec_ref, drecu_ref = loss_ref.point_losses(*[d[k] for k in ("x", "out", "knn", "res", "rec", "recu",
                                                                                       "ptsu", "inv", "mask")], G4)
    desc, keep = _point_desc(H, dev, d, dims)
    ws, terms = _point_fwd(dev, desc, dims, _counter(dev), 12345.0)
    dres, drec, drecu = _point_bwd(dev, desc, dims)
    assert math.isnan(terms_ref[3].item()) and math.isnan(terms[3].item())
    assert torch.isnan(drecu_ref).all() and torch.isnan(drecu).all()
    _within(terms[:3], terms_ref[:3], torch.tensor(_point_term_bounds(d, dims)), "point_losses_fwd terms")
    for got, ref in ((dres, dres_ref), (drec, drec_ref)):
        assert (f64(got) - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


# ---------------------------------------------------------------------------------------------
# chamfer pair bookkeeping
# ---------------------------------------------------------------------------------------------
def _cd_case(name):
    if name == "tiny":
        B, S, N, P, NP = 1, 4, 3, 2, 2
        k, counts = [2], [[1, 2]]
    elif name == "long":
        # S > P*NP, NP > 256, N > 256; sample 0 has a valid part without points; sample 1 has points
        # in a part beyond its k (a slot the part family must not weigh)
        B, S, N, P, NP = 3, 1300, 300, 4, 300
        k, counts = [4, 1, 2], [[100, 0, 150, 50], [200, 100, 0, 0], [120, 180, 0, 0]]
    else:
        # 2B(P+1) = 3400 table rows > max(2BS, 2BN) = 3200 threads' worth of points
        B, S, N, P, NP = 100, 16, 8, 16, 1
        k = [1 + b % 16 for b in range(B)]
        counts = [[N // kb + (1 if i < N % kb else 0) if i < kb else 0 for i in range(P)] for kb in k]
    g = torch.Generator().manual_seed(B)
    c = dict(dims=(B, S, N, P, NP), k=torch.tensor(k), counts=torch.tensor(counts),
             out=torch.randn(B, S, 3, generator=g), x=torch.randn(B, N, 3, generator=g), xs=torch.randn(B, N, 3, generator=g))
    c["off"], c["gid"] = loss_ref.parts_table(c["counts"], N)
    return c


def _dev(c, dev, *keys):
    return [c[k].to(dev).contiguous() for k in keys]


@pytest.mark.parametrize("name", ["tiny", "long", "tables_outnumber_points"])
def test_cd_pair_prep(H, dev, name):
    c = _cd_case(name)
    B, S, N, P, NP = c["dims"]
    out, x, xs, k, counts, off = _dev(c, dev, "out", "x", "xs", "k", "counts", "off")
    A, X2, XS2 = _filled(dev, 2 * B, S, 3), _filled(dev, 2 * B, N, 3), _filled(dev, 2 * B, N, 3)
    segf = _filled(dev, 2 * B, 4, value=-1, dtype=torch.int32)
    segp = _filled(dev, 2 * B * P, 4, value=-1, dtype=torch.int32)
    _call("ured_cd_pair_prep", _p(out), _p(x), _p(xs), _p(k), _p(counts), _p(off), B, S, N, P, NP, _p(A), _p(X2), _p(XS2),
          _p(segf), _p(segp), _stream(out))
    rA, rX2, rXS2, rf, rp = loss_ref.cd_prep(c["out"], c["x"], c["xs"], c["k"], c["counts"], c["off"], B, S, N, P, NP)
    unwritten = int((segf.cpu() == -1).all(1).sum()), int((segp.cpu() == -1).all(1).sum())
    assert unwritten == (0, 0), f"unwritten table rows (full, part): {unwritten}"
    assert torch.equal(segf.cpu(), rf) and torch.equal(segp.cpu(), rp)
    for got, ref in ((A, rA), (X2, rX2), (XS2, rXS2)):
        assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32))


def _cd_reduce(dev, c, dist, counter):
    B, S, N, P, NP = c["dims"]
    k, counts, off = _dev(c, dev, "k", "counts", "off")
    ws, terms = _filled(dev, 3 * 2 * B * (P + 1)), _filled(dev, 4)
    _call("ured_cd_pair_reduce", *[_p(v) for v in dist], _p(k), _p(counts), _p(off), B, S, N, P, NP, _p(ws), _p(counter),
          _p(terms), _stream(ws))
    assert counter.item() == 0, "the counter is not back at 0"
    return ws, terms


def _cd_dists(dev, c):
    """Random positive 'distances' of both families (no NN launch): [2BS], [2BN], [2BS], [2BN]."""
    B, S, N, P, NP = c["dims"]
    g = torch.Generator().manual_seed(S + N)
    return [(torch.rand(2 * B * m, generator=g) + 0.1).to(dev) for m in (S, N, S, N)]


def _check_cd_reduce(dev, c, counter):
    B, S, N, P, NP = c["dims"]
    dist = _cd_dists(dev, c)
    ws, terms = _cd_reduce(dev, c, dist, counter)
    ws2, terms2 = _cd_reduce(dev, c, dist, counter)
    assert torch.equal(terms.view(torch.int32), terms2.view(torch.int32)) and torch.equal(ws.view(torch.int32),
                                                                                          ws2.view(torch.int32))
    assert not torch.isnan(ws).any(), "workspace: not every element written"
    ref, longest = loss_ref.cd_reduce(*dist, c["k"], c["counts"], c["off"], B, S, N, P, NP)
    # positive terms with positive coefficients: the sum of |terms| is the value itself
    _within(terms, ref, (math.ceil(longest / 256) + 8 + 1) * U32 * ref, "cd_pair_reduce terms")


@pytest.mark.parametrize("name", ["tiny", "long"])
def test_cd_pair_reduce(H, dev, name):
    counter = _counter(dev)
    _check_cd_reduce(dev, _cd_case("long" if name == "tiny" else "tiny"), counter)     # another grid first
    _check_cd_reduce(dev, _cd_case(name), counter)


def test_cd_pair_reduce_largest_accepted(H, dev):
    """B = 128 (all 256 combining threads), the most parts whose 3 * 2B(P+1) staged floats fit: the
    entry's own cap 2B(P+1) = 8448 or the device's LDS per workgroup less the kernel's static
    arrays (>= 3072 bytes: 256 floats + 256 doubles); one more part is refused."""
    limit = torch.cuda.get_device_properties(dev).shared_memory_per_block
    B, NP = 128, 1
    counter = _counter(dev)

    def case(P):
        g = torch.Generator().manual_seed(P)
        k = torch.randint(1, P + 1, (B,), generator=g)
        counts = (torch.arange(P).unsqueeze(0) < k.unsqueeze(1)).long()
        counts[:, 0] += P - k                             # N = P points over the k_b parts
        c = dict(dims=(B, P, P, P, NP), k=k, counts=counts)
        c["off"], c["gid"] = loss_ref.parts_table(counts, P)
        return c

    accepted = None
    from ured_hip import _lib
    for P in range(34, 0, -1):
        try:
            _check_cd_reduce(dev, case(P), counter)
        except _lib.UredError:
            assert accepted is None
            continue
        accepted = P
        break
    assert accepted is not None and accepted < 34
    units = 2 * B * (accepted + 1)
    print(f"cd_pair_reduce: largest accepted 2B(P+1) = {units} (LDS per workgroup {limit} bytes)")
    assert 12 * units + 3072 <= limit
    assert units == 8448 or 12 * (units + 2 * B) + 3072 + 64 > limit, "refused although it fits"
    torch.cuda.synchronize()
    assert counter.item() == 0


@pytest.mark.parametrize("name", ["tiny", "long"])
def test_cd_pair_grad_fold(H, dev, name):
    c = _cd_case(name)
    B, S, N, P, NP = c["dims"]
    k, counts, gid = _dev(c, dev, "k", "counts", "gid")
    g4 = torch.tensor([0.7, -1.3, 2.0, 0.4])
    outs = [_filled(dev, 2 * B * m) for m in (S, N, S, N)] + [_filled(dev, 2 * B * S, 3)]
    _call("ured_cd_pair_grad", _p(g4.to(dev)), _p(k), _p(counts), _p(gid), B, S, N, P, NP, *[_p(o) for o in outs], _stream(k))
    ref = loss_ref.cd_grad(g4, c["k"], c["counts"], c["gid"], B, S, N, P, NP)
    for nm, got, r in zip(("gd_a_full", "gd_b_full", "gd_a_part", "gd_b_part"), outs, ref):
        assert not torch.isnan(got).any(), f"{nm}: not every element written"
        assert torch.equal(f64(got) == 0, r == 0), f"{nm}: zero pattern"
        nz = r != 0
        _within(got.cpu()[nz], r[nz], 4 * U32 * r[nz].abs(), "cd_pair_grad " + nm)
    assert outs[4].cpu().view(torch.int32).eq(0).all(), "ga is not all (+)zero"
    ga = torch.randn(2 * B * S, 3, generator=torch.Generator().manual_seed(S))
    gout = _filled(dev, B, S, 3)
    _call("ured_cd_pair_fold", _p(ga.to(dev)), B, S, _p(gout), _stream(gout))
    assert torch.equal(gout.cpu().view(torch.int32), loss_ref.cd_fold(ga, B, S).view(torch.int32))


# ---------------------------------------------------------------------------------------------
# loss assembly
# ---------------------------------------------------------------------------------------------
def _assemble_args(H, dev, K, T, order, w):
    ptrs = (ctypes.c_void_p * H.ASSEMBLE_MAX)(*[T.data_ptr() + 4 * i for i in order[:H.ASSEMBLE_MAX]])
    wts = (ctypes.c_float * H.ASSEMBLE_MAX)(*w[:H.ASSEMBLE_MAX])
    return ptrs, wts


@pytest.mark.parametrize("K", [1, 9, 16])
def test_assemble(H, dev, K):
    g = torch.Generator().manual_seed(K)
    T = torch.randn(20, generator=g) * 10
    order = torch.randperm(20, generator=g)[:K].tolist()
    w = (torch.randn(K, generator=g) * 5).tolist()
    Td = T.to(dev)
    ptrs, wts = _assemble_args(H, dev, K, Td, order, w)
    out, gt = _filled(dev, 1), _filled(dev, H.ASSEMBLE_MAX)
    gup = torch.tensor([-2.5], device=dev)
    _call("ured_loss_assemble", K, ptrs, wts, _p(out), _stream(out))
    _call("ured_loss_assemble_bwd", K, wts, _p(gup), _p(gt), _stream(out))
    s, gterms = loss_ref.assemble([T[i].item() for i in order], w, -2.5)
    assert out.cpu().numpy()[0].tobytes() == s.tobytes()
    assert gt.cpu().numpy()[:K].tobytes() == gterms.tobytes()
    assert torch.isnan(gt[K:]).all()


@pytest.mark.parametrize("K", [0, 17])
def test_assemble_rejects(H, dev, K):
    Td = torch.zeros(20, device=dev)
    ptrs, wts = _assemble_args(H, dev, K, Td, list(range(16)), [1.0] * 16)
    out, gt = _filled(dev, 1), _filled(dev, 20)
    gup = torch.ones(1, device=dev)
    _rejected("ured_loss_assemble", K, ptrs, wts, _p(out), _stream(out))
    _rejected("ured_loss_assemble_bwd", K, wts, _p(gup), _p(gt), _stream(out))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(gt).all()
