"""The optimizer tail (ured_adam_clip_step, csrc/optim.hip: per-module gradient clip + Adam over flat
buffers) against tests/optim_ref.py (float64; pinned to torch's clip_grad_norm_ + Adam by
tests/test_optim_ref.py), one launch at a time from a known state, at what the step-level tests
never reach: clip and Adam together element by element, the unclipped branch next to a clipped
segment, segments of more than 256 chunks, segments and launches without an active parameter,
inactive parameters holding stale gradients inside a clipped segment, sizes around the layout
constants (1, 5, 16, 17, 8192, 8193, 2*8192+4) with their zero padding, step counts up to 100000
mixed in one launch, max_norm = 0, non-finite gradients, the argument checks. The kernel-level
tests call the entry through _lib.call with tables built by optim_ref.chunk_tables from the header's
contract (ured_hip.optim is imported for the registered signature only); the FlatAdam-level test
drives FlatAdam.step(max_norm=5) for six steps, each compared from the GPU's own previous state.

Inputs: parameters of order 1, gradients of order 1e-3 .. 1e3, first moments of the gradients'
order and second moments >= 0.05 * (that order)^2 (or both exactly zero), so no intermediate of
the kernel is subnormal in fp32 and no comparison depends on flush-to-zero behaviour. Every case
asserts on the reference that |norm / max_norm - 1| >= 1e-3 in every non-empty segment: none sits
on the clip branch and no element is left out of any comparison.

Tolerances (u = 2^-24; every bound is computed per element from the float64 reference's values and
multiplied by 1.001, which covers the second-order terms and the fp64 evaluation errors)
  The kernel evaluates each expression in double and rounds to float at these points; the
  element-wise comparison uses the coefficients read back from the GPU (coef= of the reference), so
  it is independent of the norm:
    gc = fl(g*coef)                      e_g  = u|gc|                                  (1 rounding)
    gw = fl(gc + wd*p)                   e_gw = e_g + u|gw|                            (2)
    m' = fl(b1*m + (1-b1)*gw)            e_m  = (1-b1) e_gw + u|m'|                    (<= 3 of |m'| on a first step)
    v' = fl(b2*v + (1-b2)*gw^2)          e_v  = 2(1-b2)|gw| e_gw + u|v'|               (<= 5 of |v'| on a first step)
    denom = fl(fl(sqrtf(v')/bc2s) + eps) r_den = e_v/(2v') + u [sqrtf] + 2u [bc2s = sqrtf(fl(1-b2^t)), rounded
                                                 twice] + u [the division] + u [adding eps]      (<= 7.5)
    p' = fl(p - lr/bc1 * m'/denom)       e_p  = |lr/bc1/denom| e_m + |update| (r_den + u [bc1]) + u|p'|
  i.e. 2^-24 |p'| for the final store plus k * 2^-24 |update| with k <= 3 + 7.5 + 1 = 11.5 where
  nothing cancels (k is largest on a parameter's first step, when m and v hold only this gradient).
  sqrtf and the float division are correctly rounded (hipcc's default), pow is evaluated in double.
  A gradient that is not written back (max_norm <= 0) and everything about an inactive parameter or
  the padding is compared bitwise.
  Clip coefficient, by the rule of test_loss_kernels_gpu.py for fp32 sums of non-negative terms:
  (per-thread run + tree levels + extra) u on the sum of squares = (8 + 0 + 2) u: 8 = CHUNK/(4*256)
  accumulations of a thread per chunk, 0 because the trees over the threads and over the chunks run
  in double, 2 for a square and the add of two squares; halved by the square root (5u), plus the float
  roundings of norm, norm + 1e-6f and the division: 8u relative, and exactly 1 where the reference
  does not clip (plus u * 1e-6 / norm for 1e-6f != 1e-6).

Measured on MI355X (worst error / bound over all cases of this file, about 5 million elements):
  coef 0.109   g 0.994   m 0.994   v 0.998   p 0.998
  g, m, v and p come close to 1 because for many elements one rounding carries the whole bound (g has
  only one; a large b2*v next to a small gradient, a parameter much larger than its update) and
  half an ulp is reached among millions of elements; none exceeds it. With the kernel as it was
  before this test (fminf for the clamp) test_nan_gradient_propagates_as_in_clip_grad_norm fails
  with coef = 1 where the reference's is nan; every other test passes on both.
"""
import numpy as np
import pytest
import torch

import optim_ref
from optim_ref import ALIGN, CHUNK, U32, adam_clip_step_ref, chunk_tables

pytestmark = pytest.mark.gpu

HYP = dict(b1=0.9, b2=0.999, eps=1e-8, wd=5e-4)
LR = 1e-3
MAX_NORM = 5.0
SLACK = 1.001
COEF_ROUNDINGS = (CHUNK // (4 * optim_ref.LT) + 0 + 2) / 2 + 3        # 8, see the docstring
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def lib(dev):
    from ured_hip import _lib, optim          # noqa: F401  (optim registers the entry point's signature)
    return _lib


def _note(name, ratio):
    """Running worst error / bound of a quantity (printed: pytest -s shows it)."""
    if ratio > WORST.get(name, -1.0):
        WORST[name] = ratio
        print(f"optim {name}: worst error / bound so far {ratio:.3f}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


class Layout:
    """Parameters of `sizes` in segments `seg_of`, laid out and chunked by optim_ref.chunk_tables."""

    def __init__(self, sizes, seg_of, active, nseg=None):
        self.sizes, self.seg_of, self.active = list(sizes), list(seg_of), [bool(a) for a in active]
        self.T = chunk_tables(sizes, seg_of, active, nseg=nseg)
        self.n, self.nseg, self.total, self.off = len(sizes), self.T["nseg"], self.T["total"], self.T["offsets"]
        self.nchunks = len(self.T["chunk_beg"])
        self.padded = [-(-s // ALIGN) * ALIGN for s in sizes]

    def pack(self, arrs):
        flat = np.zeros(self.total, dtype=np.float32)
        for o, s, a in zip(self.off, self.sizes, arrs):
            flat[o:o + s] = a
        return flat

    def split(self, flat):
        return [flat[o:o + s] for o, s in zip(self.off, self.sizes)]

    def padding(self, flat, i):
        return flat[self.off[i] + self.sizes[i]:self.off[i] + self.padded[i]]

    def tables(self, dev):
        def t(key):                     # an empty table still gets a valid pointer
            a = self.T[key]
            return torch.from_numpy(a if len(a) else np.zeros(1, dtype=a.dtype)).to(dev)
        return {k: t(k) for k in ("chunk_beg", "chunk_end", "chunk_seg", "chunk_param", "seg_chunk0",
                                        "active_params")}


def _state(lay, seed, gscale=1.0, steps=0, zero_gm=False, norms=None):
    """fp32 p, g, m, v per parameter and the step counts; gscale / steps: scalars or one per
    parameter; norms: {segment: float64 norm its active gradients are scaled to}."""
    rng = np.random.default_rng(seed)
    gs = np.broadcast_to(np.asarray(gscale, dtype=np.float64), (lay.n,))
    st = dict(p=[], g=[], m=[], v=[], step=np.broadcast_to(np.asarray(steps, np.float32), (lay.n,)).copy())
    for n, s in zip(lay.sizes, gs):
        st["p"].append(rng.standard_normal(n).astype(np.float32))
        st["g"].append((s * rng.standard_normal(n)).astype(np.float32))
        st["m"].append((0.3 * s * rng.standard_normal(n)).astype(np.float32))
        st["v"].append((s * s * (0.05 + rng.random(n))).astype(np.float32))
        if zero_gm:
            for k in ("g", "m", "v"):
                st[k][-1][:] = 0
    for seg, target in (norms or {}).items():
        _set_norm(st, lay, seg, target)
    return st


def _set_norm(st, lay, seg, target):
    """Scale the active gradients of segment `seg` so that their float64 norm is `target`."""
    idx = [i for i in range(lay.n) if lay.seg_of[i] == seg and lay.active[i]]
    nrm = np.sqrt(sum(np.sum(st["g"][i].astype(np.float64) ** 2) for i in idx))
    for i in idx:
        st["g"][i] = (st["g"][i].astype(np.float64) * (target / nrm)).astype(np.float32)


class Device:
    """The flat buffers, tables and scalars of one layout on the GPU."""

    def __init__(self, dev, lay, st, lr=LR):
        self.lay, self.dev = lay, dev
        # 16 floats of room behind every buffer (the rejection tests offset a pointer)
        self.buf = {k: torch.from_numpy(np.concatenate([lay.pack(st[k]), np.zeros(16, np.float32)])).to(dev)
                    for k in "pgmv"}
        self.step = torch.from_numpy(st["step"].astype(np.float32)).to(dev)
        self.tab = lay.tables(dev)
        self.lr = torch.tensor([lr], dtype=torch.float32, device=dev)
        self.coef = torch.full((max(lay.nseg, 1),), NAN, device=dev)
        self.partial = torch.full((max(lay.nchunks, 1),), NAN, dtype=torch.float64, device=dev)

    def args(self, max_norm, hyp=HYP, **over):
        from ured_hip import _lib
        b, t, lay = self.buf, self.tab, self.lay
        a = dict(param=b["p"].data_ptr(), grad=b["g"].data_ptr(), exp_avg=b["m"].data_ptr(),
                 exp_avg_sq=b["v"].data_ptr(), chunk_beg=t["chunk_beg"].data_ptr(),
                 chunk_end=t["chunk_end"].data_ptr(), chunk_seg=t["chunk_seg"].data_ptr(),
                 chunk_param=t["chunk_param"].data_ptr(), nchunks=lay.nchunks,
                 seg_chunk0=t["seg_chunk0"].data_ptr(), nseg=lay.nseg, max_norm=float(max_norm),
                 lr=self.lr.data_ptr(), param_step=self.step.data_ptr(),
                 active_params=t["active_params"].data_ptr(), n_active=len(lay.T["active_params"]),
                 beta1=hyp["b1"], beta2=hyp["b2"], eps=hyp["eps"], weight_decay=hyp["wd"],
                 partial=self.partial.data_ptr(), coef=self.coef.data_ptr(), stream=_lib.stream_of(b["p"]))
        a.update(over)
        return list(a.values())

    def launch(self, max_norm, hyp=HYP, **over):
        from ured_hip import _lib
        _lib.call("ured_adam_clip_step", *self.args(max_norm, hyp, **over))

    def set_grads(self, grads):
        """This step's gradients of the active parameters (the others keep what they hold)."""
        g = self.buf["g"].cpu().numpy().copy()
        for i, a in enumerate(self.lay.active):
            if a:
                g[self.lay.off[i]:self.lay.off[i] + self.lay.sizes[i]] = grads[i]
        self.buf["g"].copy_(torch.from_numpy(g))

    def host(self):
        """fp32 host copies: flat p, g, m, v (without the spare room), step, coef, partial."""
        h = {k: self.buf[k].cpu().numpy()[:self.lay.total].copy() for k in "pgmv"}
        h.update(step=self.step.cpu().numpy().copy(), coef=self.coef.cpu().numpy().copy(),
                 partial=self.partial.cpu().numpy().copy())
        return h


def _bounds(p, g, m, v, t, cf, lr, b1, b2, eps, wd):
    """Per-element rounding bounds of one step (see the module docstring) from float64 values."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        gc = g * cf
        gw = gc + wd * p
        m1 = b1 * m + (1 - b1) * gw
        v1 = b2 * v + (1 - b2) * gw * gw
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        den = np.sqrt(v1) / np.sqrt(bc2) + eps
        k = lr / bc1 / den
        upd = k * m1
        e_g = U32 * np.abs(gc)
        e_gw = e_g + U32 * np.abs(gw)
        e_m = (1 - b1) * e_gw + U32 * np.abs(m1)
        e_v = 2 * (1 - b2) * np.abs(gw) * e_gw + U32 * np.abs(v1)
        r_den = np.where(v1 > 0, e_v / (2 * np.where(v1 > 0, v1, 1.0)), 0.0) + 5 * U32
        e_p = np.abs(k) * e_m + np.abs(upd) * (r_den + U32) + U32 * np.abs(p - upd)
    return dict(g=SLACK * e_g, m=SLACK * e_m, v=SLACK * e_v, p=SLACK * e_p)


def _within(got, ref, bound, name, tag):
    got = got.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag} {name}: nan positions differ from the reference's"
    ok = ~np.isnan(ref)
    if not ok.any():
        return
    err, bnd = np.abs(got[ok] - ref[ok]), bound[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bnd)
    _note(name, float(ratio.max()))
    bad = err > bnd
    assert not bad.any(), (f"{tag} {name}: {int(bad.sum())} elements over the rounding bound, worst error / bound "
                           f"{ratio.max():.3f} (error {err[np.argmax(ratio)]:.3e})")


def _compare(lay, before, after, fresh_g, max_norm, lr, hyp=HYP, tag=""):
    """One launch: `before` / `after` are Device.host() copies, fresh_g the per-parameter gradients
    the launch read (for the active parameters). Checks coef against the reference's own, every
    active element against the reference run with the GPU's coef, everything else bitwise."""
    lr = float(np.float32(lr))
    sp = {k: lay.split(before[k]) for k in "pgmv"}
    sa = {k: lay.split(after[k]) for k in "pgmv"}
    w = {k: [x.astype(np.float64) for x in sp[k]] for k in "pmv"}
    g64 = [np.asarray(x, dtype=np.float32).astype(np.float64) for x in fresh_g]
    own = adam_clip_step_ref(w["p"], g64, w["m"], w["v"], before["step"], lay.seg_of, lay.active, max_norm, lr,
                             nseg=lay.nseg, **hyp)
    coef = after["coef"][:lay.nseg]
    # -- the clip coefficient
    for s in range(lay.nseg):
        nrm, c = own["norm"][s], own["coef"][s]
        empty = not any(lay.active[i] and lay.seg_of[i] == s for i in range(lay.n))
        if max_norm <= 0 or empty:
            assert coef[s] == 1.0, f"{tag}: coef[{s}] = {coef[s]} (no clipping, or no active parameter)"
        elif np.isnan(c):
            assert np.isnan(coef[s]), f"{tag}: coef[{s}] = {coef[s]}, the reference's is nan"
        else:
            if np.isfinite(nrm):
                assert abs(nrm / max_norm - 1) >= 1e-3, f"{tag}: segment {s} sits on the clip branch"
            if c == 1.0 or c == 0.0:
                assert coef[s] == c, f"{tag}: coef[{s}] = {coef[s]!r}, expected exactly {c}"
            else:
                bound = SLACK * (COEF_ROUNDINGS * U32 + U32 * 1e-6 / nrm) * c
                err = abs(float(coef[s]) - c)
                _note("coef", err / bound)
                assert err <= bound, f"{tag}: coef[{s}] off by {err:.3e} > {bound:.3e} ({err / bound:.2f} x)"
    # -- the elements, with the GPU's coefficients
    ref = adam_clip_step_ref(w["p"], g64, w["m"], w["v"], before["step"], lay.seg_of, lay.active, max_norm, lr,
                             coef=coef.astype(np.float64), nseg=lay.nseg, **hyp)
    assert np.array_equal(after["step"], before["step"] + np.asarray(lay.active, np.float32)), f"{tag}: step counts"
    assert np.array_equal(after["step"].astype(np.float64), ref["step"])
    for i in range(lay.n):
        t = f"{tag} parameter {i} ({lay.sizes[i]})"
        if not lay.active[i]:
            for k in "pgmv":
                assert _same_bits(sa[k][i], sp[k][i]), f"{t}: inactive, yet {k} changed"
                assert _same_bits(lay.padding(after[k], i), lay.padding(before[k], i)), f"{t}: inactive, {k} padding"
            continue
        cf = float(coef[lay.seg_of[i]])
        b = _bounds(w["p"][i], g64[i], w["m"][i], w["v"][i], ref["step"][i], cf, lr, **hyp)
        if max_norm > 0:
            _within(sa["g"][i], ref["g"][i], b["g"], "g", t)
        else:
            assert _same_bits(sa["g"][i], sp["g"][i]), f"{t}: max_norm <= 0, yet the gradient was written"
        for k in "mvp":
            _within(sa[k][i], ref[k][i], b[k], k, t)
        if np.isfinite(cf):
            for k in "pgmv":
                assert (lay.padding(after[k], i) == 0).all(), f"{t}: {k} padding is not zero"
    return own, ref


def _launch_and_compare(dev, lay, st, max_norm=MAX_NORM, lr=LR, hyp=HYP, launches=1, regrad=None, tag=""):
    """`launches` launches in a row on one device state, each compared from the GPU's previous
    state; regrad(n) gives launch n > 0 its fresh gradients (a clipped gradient left in place would
    put the next norm on the branch)."""
    d = Device(dev, lay, st, lr)
    out = None
    for n in range(launches):
        if n:
            d.set_grads(regrad(n))
        before = d.host()
        d.launch(max_norm, hyp)
        after = d.host()
        out = _compare(lay, before, after, lay.split(before["g"]), max_norm, lr, hyp, f"{tag} launch {n}")
    return d, out


# ---------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------
SIZES = [1, 5, 16, 17, 8192, 8193, 2 * 8192 + 4]
SIZES_SEG = [0, 0, 0, 1, 1, 2, 2]


def test_sizes_around_the_layout_constants(lib, dev):
    """The size list over three segments at the workload's hyper-parameters, gradient scales 1e-2 ..
    1e2 mixed inside a segment; three launches in a row, each compared from the GPU's previous
    state, the padding exactly zero in all four buffers after each."""
    lay = Layout(SIZES, SIZES_SEG, [True] * 7)

    def state(n):
        return _state(lay, 1 + 100 * n, gscale=[1e2, 1e-2, 1.0, 1e-2, 1e-3, 10.0, 1e-2], steps=[0, 3, 7, 1, 0, 2, 12],
                      norms={0: 8 * MAX_NORM, 1: 0.4 * MAX_NORM})       # segment 2 as it comes: about 180 max_norm
    d, (own, _) = _launch_and_compare(dev, lay, state(0), launches=3, regrad=lambda n: state(n)["g"], tag="sizes")
    assert own["coef"][0] < 1 and own["coef"][1] == 1 and own["coef"][2] < 1
    h = d.host()
    used = np.zeros(lay.total, bool)
    for o, s in zip(lay.off, lay.sizes):
        used[o:o + s] = True
    for k in "pgmv":
        assert (h[k][~used] == 0).all(), f"{k}: padding not zero after three launches"
        assert (d.buf[k][lay.total:] == 0).all()


def test_three_clip_regimes_and_long_segments(lib, dev):
    """Segment 0: 300 sixteen-element parameters (300 chunks: the second trip of seg_coef_kernel's
    loop) at 0.3 max_norm, not clipped. Segment 1: one parameter of 300 * 8192 elements (a parameter
    over many chunks) at 20 max_norm, clipped. Segment 2: one parameter without a gradient."""
    sizes = [16] * 300 + [300 * CHUNK, 40]
    seg_of = [0] * 300 + [1, 2]
    lay = Layout(sizes, seg_of, [True] * 301 + [False])
    assert lay.nchunks == 600 and list(lay.T["seg_chunk0"]) == [0, 300, 600, 600]
    st = _state(lay, 2, gscale=1.0, steps=4, norms={0: 0.3 * MAX_NORM, 1: 20 * MAX_NORM})
    d, (own, _) = _launch_and_compare(dev, lay, st, tag="regimes")
    assert list(own["coef"][[0, 2]]) == [1.0, 1.0] and abs(own["coef"][1] - 0.05) < 1e-6
    assert d.host()["coef"][0] == 1.0 and d.host()["coef"][2] == 1.0


@pytest.mark.parametrize("wd", [5e-4, 0.0])
def test_step_counts_mixed_in_one_launch(lib, dev, wd):
    """Step counts 0, 5, 1000 and 100000 before the launch on different parameters (the bias
    correction 1 - 0.9^t rounds to 1 in fp32 from t = 165 on; 1 - 0.999^t from t = 17321 on)."""
    hyp = dict(HYP, wd=wd)
    sizes = [40, 17, CHUNK + 1, 5, 64, 16]
    lay = Layout(sizes, [0, 0, 1, 1, 1, 0], [True] * 6)

    def state(n):
        return _state(lay, 3 + 100 * n, gscale=[1.0, 10.0, 1.0, 1e-2, 1.0, 1.0],
                      steps=[0, 100000, 5, 1000, 100000, 1000], norms={1: 0.5 * MAX_NORM})
    d, _ = _launch_and_compare(dev, lay, state(0), hyp=hyp, launches=2, regrad=lambda n: state(n)["g"],
                               tag=f"steps wd={wd}")
    assert list(d.host()["step"]) == [2, 100002, 7, 1002, 100002, 1002]


def test_zero_gradient_zero_moments_no_decay_is_no_update(lib, dev):
    lay = Layout([5, 17, CHUNK + 3], [0, 0, 1], [True] * 3)
    st = _state(lay, 4, zero_gm=True, steps=[0, 9, 1000])
    d = Device(dev, lay, st)
    before = d.host()
    d.launch(MAX_NORM, dict(HYP, wd=0.0))
    after = d.host()
    for k in "pgmv":
        assert _same_bits(after[k], before[k]), f"{k} changed"
    assert (after["coef"] == 1).all() and list(after["step"]) == [1, 10, 1001]


def test_inactive_parameters_with_stale_gradients(lib, dev):
    """Inactive parameters inside a clipped segment hold non-zero gradients, moments and step
    counts: bitwise untouched, and outside the norm (the coefficient is the reference's, which is
    computed without them; with them the norm would be 50 times larger)."""
    sizes = [64, 33, CHUNK + 5, 16, 7, 300]
    seg_of = [0, 0, 0, 0, 1, 1]
    active = [True, False, False, True, True, False]
    lay = Layout(sizes, seg_of, active)

    def state(n):
        return _state(lay, 5 + 100 * n, gscale=[1.0, 50.0, 50.0, 1.0, 1.0, 50.0], steps=[3, 8, 2, 3, 0, 11],
                      norms={0: 3 * MAX_NORM, 1: 2 * MAX_NORM})
    d, (own, _) = _launch_and_compare(dev, lay, state(0), launches=2, regrad=lambda n: state(n)["g"], tag="stale")
    assert abs(own["coef"][0] - 1 / 3) < 1e-6 and abs(own["coef"][1] - 0.5) < 1e-6
    assert list(d.host()["step"]) == [5, 8, 2, 5, 2, 11]


def test_max_norm_zero_leaves_the_gradient(lib, dev):
    lay = Layout(SIZES, SIZES_SEG, [True, True, False, True, True, True, True])
    st = _state(lay, 6, gscale=100.0, steps=2)
    d, _ = _launch_and_compare(dev, lay, st, max_norm=0.0, tag="max_norm 0")
    h = d.host()
    assert (h["coef"] == 1).all() and _same_bits(h["g"], lay.pack(st["g"]))


@pytest.mark.parametrize("max_norm", [MAX_NORM, 0.0])
def test_no_chunks_no_active_parameter(lib, dev, max_norm):
    lay = Layout([5, 40, CHUNK + 1], [0, 1, 1], [False] * 3, nseg=3)
    assert lay.nchunks == 0 and len(lay.T["active_params"]) == 0
    st = _state(lay, 7, gscale=10.0, steps=[1, 2, 3])
    d = Device(dev, lay, st)
    before = d.host()
    d.launch(max_norm)
    after = d.host()
    for k in ("p", "g", "m", "v", "step"):
        assert _same_bits(after[k], before[k]), f"{k} changed"
    assert (after["coef"] == 1).all()


def test_same_launch_twice_is_bitwise_equal(lib, dev):
    sizes = [16] * 270 + [3 * CHUNK + 4, 17]
    lay = Layout(sizes, [0] * 270 + [1, 1], [True] * 272)
    st = _state(lay, 8, gscale=1.0, steps=1, norms={0: 4 * MAX_NORM})
    out = []
    for _ in range(2):
        d = Device(dev, lay, st)
        d.launch(MAX_NORM)
        out.append(d.host())
    for k in ("p", "g", "m", "v", "step", "coef", "partial"):
        assert _same_bits(out[0][k], out[1][k]), f"{k} differs between two identical launches"
    assert not np.isnan(out[0]["partial"]).any() and (out[0]["coef"] < 1).all()


def test_argument_checks(lib, dev):
    """nseg = 64 is accepted and 65 is not; a null lr; a flat buffer that is not 16-byte aligned.
    Nothing is launched by a rejected call: the state is bitwise what it was."""
    lay = Layout([5, 33], [0, 63], [True, True], nseg=64)
    st = _state(lay, 9, steps=1)
    d = Device(dev, lay, st)
    d.launch(MAX_NORM)                                     # 64 segments: accepted
    h = d.host()
    assert not np.isnan(h["coef"]).any() and list(h["step"]) == [2, 2]
    # 65: tables long enough for it, so that the refusal is about nseg alone
    seg0 = torch.cat([d.tab["seg_chunk0"], d.tab["seg_chunk0"][-1:]])
    coef = torch.ones(65, device=dev)
    for over in (dict(nseg=65, seg_chunk0=seg0.data_ptr(), coef=coef.data_ptr()), dict(lr=None),
                 dict(param=d.buf["p"].data_ptr() + 4), dict(exp_avg_sq=d.buf["v"].data_ptr() + 4)):
        with pytest.raises(lib.UredError):
            d.launch(MAX_NORM, **over)
    after = d.host()
    for k in ("p", "g", "m", "v", "step", "coef"):
        assert _same_bits(after[k], h[k]), f"a rejected call changed {k}"


def _three_segments(seed):
    sizes = [40, 17, CHUNK + 1, 64, 5, 33, 16]
    seg_of = [0, 0, 1, 1, 1, 2, 2]
    lay = Layout(sizes, seg_of, [True, True, True, True, False, True, True])
    return lay, _state(lay, seed, gscale=1.0, steps=[0, 4, 2, 2, 6, 1, 9],
                       norms={0: 6 * MAX_NORM, 1: 3 * MAX_NORM, 2: 0.2 * MAX_NORM})


def test_nan_gradient_propagates_as_in_clip_grad_norm(lib, dev):
    """One nan gradient element in segment 1: torch's clamp(max_norm / (norm + 1e-6), max=1) is nan,
    so the segment's coefficient is nan and every active element of it comes back nan in g and p
    (and m, v); its inactive parameter and the other segments are as without the nan."""
    lay, st = _three_segments(10)
    st["g"][3][7] = NAN
    d, (own, _) = _launch_and_compare(dev, lay, st, tag="nan")
    h = d.host()
    assert np.isnan(own["coef"][1]) and np.isnan(h["coef"][1]) and np.isfinite(h["coef"][[0, 2]]).all()
    for k in "gpmv":
        sp = lay.split(h[k])
        for i in range(lay.n):
            if lay.seg_of[i] == 1 and lay.active[i]:
                assert np.isnan(sp[i]).all(), f"{k} of parameter {i} is not all nan"
            else:
                assert np.isfinite(sp[i]).all(), f"{k} of parameter {i} (another segment, or inactive)"


def test_infinite_norm_gives_coefficient_zero(lib, dev):
    """One infinite gradient element: norm = inf, coef = max_norm / inf = 0 exactly; the segment's
    gradients come back 0 but for inf * 0 = nan at that element, as with clip_grad_norm_."""
    lay, st = _three_segments(11)
    st["g"][2][CHUNK] = np.inf                             # the last element, in the second chunk
    d, (own, _) = _launch_and_compare(dev, lay, st, tag="inf")
    h = d.host()
    assert own["coef"][1] == 0 and h["coef"][1] == 0 and (h["coef"][[0, 2]] > 0).all()
    g = lay.split(h["g"])
    assert np.isnan(g[2][CHUNK]) and (g[2][:CHUNK] == 0).all() and (g[3] == 0).all()
    assert np.isnan(lay.split(h["p"])[2][CHUNK]) and np.isfinite(lay.split(h["p"])[2][:CHUNK]).all()


# ---------------------------------------------------------------------------------------------
# FlatAdam level
# ---------------------------------------------------------------------------------------------
def test_flat_adam_six_clipped_steps(lib, dev):
    """FlatAdam.step(max_norm=5) for six steps on a dozen parameters in three segments: segment 0
    always clipped, segment 1 never, segment 2 never with a gradient; parameter 3 joins at step 2 (it
    lies behind the others in the flat layout), parameter 0 leaves after step 2 (its slice of the
    flat gradient keeps the clipped gradient of step 2); lr changes at step 3. Before every step p,
    m, v and the step counts are read back from the GPU and fed to the reference, so the
    single-step bounds of the module docstring apply to every step."""
    from ured_hip.optim import FlatAdam
    shapes = [(64, 3), (64,), (17,), (CHUNK + 1,), (5,), (16, 16), (1,), (33, 7), (7, 7), (3,), (9, 2), (4,)]
    seg_of = [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    gscale = [2.0, 30.0, 1.0, 1.0, 1e-2, 1e-2, 1e-2, 1e-2, 0, 0, 0, 0]
    n = len(shapes)
    gen = torch.Generator().manual_seed(12)
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(dev)) for s in shapes]
    segs = [[p for p, s in zip(params, seg_of) if s == k] for k in range(3)]
    opt = FlatAdam(params, segs, lr=LR, betas=(HYP["b1"], HYP["b2"]), eps=HYP["eps"], weight_decay=HYP["wd"])
    sizes = [p.numel() for p in params]
    count = np.zeros(n)

    def slices(flat):
        return [flat[p._ured_gslot[1]:p._ured_gslot[1] + p._ured_gslot[2]].cpu().numpy().copy() for p in params]

    for it in range(6):
        lr = LR if it < 3 else 2.5e-4
        opt.param_groups[0]["lr"] = lr
        active = [seg_of[i] < 2 and (i != 3 or it >= 2) and (i != 0 or it <= 2) for i in range(n)]
        opt.zero_grad()
        fresh = [(gscale[i] * torch.randn(*shapes[i], generator=gen)).float() for i in range(n)]
        for i in range(n):
            if active[i]:
                params[i].grad = fresh[i].clone().to(dev)
        assert list(opt.prepare()) == active
        assert all(a is b for a, b in zip(opt.params_all, params))
        lay = Layout(sizes, seg_of, active, nseg=3)
        lay.off = [p._ured_gslot[1] for p in params]       # FlatAdam's own layout
        lay.total = opt.flat_param.numel()
        if it == 0:
            assert lay.off[3] > max(lay.off[i] for i in range(n) if active[i])
        before = {k: v.cpu().numpy().copy() for k, v in
                  dict(p=opt.flat_param, g=opt.flat_grad, m=opt.state["flat"]["exp_avg"],
                       v=opt.state["flat"]["exp_avg_sq"], step=opt.state["flat"]["step"]).items()}
        assert np.array_equal(before["step"], count)
        opt.step(max_norm=MAX_NORM)
        after = {k: v.cpu().numpy().copy() for k, v in
                 dict(p=opt.flat_param, g=opt.flat_grad, m=opt.state["flat"]["exp_avg"],
                      v=opt.state["flat"]["exp_avg_sq"], step=opt.state["flat"]["step"], coef=opt._coef).items()}
        # the stale slices of inactive parameters are in `before`; the active ones read `fresh`
        g_read = [fresh[i].numpy().reshape(-1) if active[i] else lay.split(before["g"])[i] for i in range(n)]
        before["g"] = before["g"].copy()
        for i in range(n):
            if active[i]:
                before["g"][lay.off[i]:lay.off[i] + sizes[i]] = g_read[i]
        own, ref = _compare(lay, before, after, g_read, MAX_NORM, lr, tag=f"FlatAdam step {it}")
        assert own["coef"][0] < 0.5 and own["coef"][1] == 1 and own["coef"][2] == 1
        count += np.asarray(active, dtype=np.float64)
        assert np.array_equal(after["step"], count), "per-parameter step counts"
        gs = slices(opt.flat_grad)
        for i, p in enumerate(params):
            if active[i]:
                o = p._ured_gslot[1]
                assert p.grad.data_ptr() == opt.flat_grad[o:].data_ptr() and p.grad.shape == p.shape
                assert _same_bits(p.grad.cpu().numpy().reshape(-1), gs[i])      # the clipped gradient (checked above)
                assert p.data_ptr() == opt.flat_param[o:].data_ptr()
            else:
                assert p.grad is None
        if it == 3:     # parameter 0 left: its slice still holds step 2's clipped gradient, non-zero
            assert np.abs(gs[0]).max() > 0
    assert list(count) == [3, 6, 6, 4, 6, 6, 6, 6, 0, 0, 0, 0]
