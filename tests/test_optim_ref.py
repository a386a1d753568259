"""tests/optim_ref.py (the float64 restatement and the chunk tables the optimizer-tail kernel tests
compare with) against something independent: torch.nn.utils.clip_grad_norm_ per module followed by
torch.optim.Adam(weight_decay=wd) on float64 parameters, the table contract of include/ured_hip.h
as properties, and FlatAdam._set_active on CPU tensors (the layout and the tables are host logic;
only FlatAdam.step needs the GPU). Float64 against float64 agrees to 1e-12 relative, nan positions
identical. Runs on the CPU."""
import numpy as np
import pytest
import torch

import optim_ref
from optim_ref import adam_clip_step_ref, chunk_tables

RTOL = 1e-12
HYP = dict(b1=0.9, b2=0.999, eps=1e-8, wd=5e-4)
MAX_NORM = 5.0

#          0       1      2      3       4      5     6     7
SHAPES = [(8, 3), (17,), (5,), (33,), (4, 4), (1,), (7,), (2, 3)]
SEG_OF = [0, 0, 0, 0, 1, 1, 2, 2]       # segment 0 is clipped, 1 is not, 2 never has a gradient
GSCALE = [3.0, 3.0, 3.0, 3.0, 0.1, 0.1, 0.0, 0.0]
JOINS, LEAVES = 3, 2                    # parameter 3 joins at step 2, parameter 2 leaves after step 2


def _active(it):
    return [i < 6 and (i != JOINS or it >= 2) and (i != LEAVES or it <= 2) for i in range(len(SHAPES))]


def _same(got, ref, name, rtol=RTOL):
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{name}: nan positions differ"
    ok = ~np.isnan(ref)
    if ok.any():
        scale = max(np.abs(ref[ok]).max(), 1e-300)
        err = np.abs(got[ok] - ref[ok]).max()
        assert err <= rtol * scale, f"{name}: {err:.3e} > {rtol:.0e} * {scale:.3e}"


def _run(nan_at=None, steps=6):
    """`steps` steps of torch (clip per module, Adam) and of the reference side by side from the
    same float64 start, compared after every step. nan_at = (step, parameter): one nan gradient
    element there."""
    gen = torch.Generator().manual_seed(11)
    base = [torch.randn(*s, generator=gen, dtype=torch.float64) for s in SHAPES]
    tp = [torch.nn.Parameter(b.clone()) for b in base]
    mods = [[p for p, s in zip(tp, SEG_OF) if s == k] for k in range(3)]
    opt = torch.optim.Adam(tp, lr=1e-3, betas=(HYP["b1"], HYP["b2"]), eps=HYP["eps"], weight_decay=HYP["wd"])
    n = len(SHAPES)
    P = [b.numpy().reshape(-1).copy() for b in base]
    G = [np.full(P[i].size, 123.0) for i in range(n)]          # stale values: must never be read
    M = [np.zeros_like(x) for x in P]
    V = [np.zeros_like(x) for x in P]
    step = np.zeros(n)
    norms = []
    for it in range(steps):
        lr = 1e-3 if it < 3 else 2.5e-4
        opt.param_groups[0]["lr"] = lr
        act = _active(it)
        for i in range(n):
            tp[i].grad = None
            if act[i]:
                g = GSCALE[i] * torch.randn(*SHAPES[i], generator=gen, dtype=torch.float64)
                if nan_at == (it, i):
                    g.view(-1)[g.numel() // 2] = float("nan")
                tp[i].grad = g.clone()
                G[i] = g.numpy().reshape(-1).copy()
        before = [x.copy() for x in P], [x.copy() for x in M], [x.copy() for x in V], step.copy()
        stale = [x.copy() for x in G]
        for mod in mods:
            torch.nn.utils.clip_grad_norm_(mod, MAX_NORM)
        opt.step()
        r = adam_clip_step_ref(P, G, M, V, step, SEG_OF, act, MAX_NORM, lr, **HYP)
        P, G, M, V, step = r["p"], r["g"], r["m"], r["v"], r["step"]
        norms.append(r["norm"])
        for i in range(n):
            tag = f"step {it} parameter {i}"
            _same(tp[i].detach().numpy(), P[i], tag + " p")
            if act[i]:
                st = opt.state[tp[i]]
                _same(st["exp_avg"].numpy(), M[i], tag + " m")
                _same(st["exp_avg_sq"].numpy(), V[i], tag + " v")
                _same(tp[i].grad.numpy(), G[i], tag + " g")
                assert float(st["step"]) == step[i], tag
            else:       # untouched: bitwise, the stale gradient included, and no step
                assert np.array_equal(P[i], before[0][i]) and np.array_equal(M[i], before[1][i]), tag
                assert np.array_equal(V[i], before[2][i]) and np.array_equal(G[i], stale[i]), tag
                assert step[i] == before[3][i], tag
                if tp[i] in opt.state and "step" in opt.state[tp[i]]:
                    assert float(opt.state[tp[i]]["step"]) == step[i], tag
    return norms, step, P


def test_reference_matches_torch_clip_and_adam():
    norms, step, _ = _run()
    for nm in norms:            # the three regimes, away from the branch
        assert nm[0] > 1.5 * MAX_NORM and 0 < nm[1] < 0.5 * MAX_NORM and nm[2] == 0
    assert list(step) == [6, 6, 3, 4, 6, 6, 0, 0]


def test_reference_nan_gradient_matches_torch():
    """One nan gradient element makes the module's coefficient nan (clamp propagates it), hence
    all of its gradients and, after Adam, its parameters; the other module stays finite."""
    norms, _, P = _run(nan_at=(1, 1), steps=3)
    assert np.isnan(norms[1][0]) and np.isfinite(norms[1][1])
    for i in (0, 1, 2):
        assert np.isnan(P[i]).all()
    assert np.isfinite(P[3]).all()          # joined at step 2, whose gradients are finite again
    for i in (4, 5, 6, 7):
        assert np.isfinite(P[i]).all()


def test_clip_coefs_edges():
    c = optim_ref.clip_coefs(np.array([0.0, 1.0, 5.0, 50.0, np.inf, np.nan]), 5.0)
    assert c[0] == 1 and c[1] == 1 and c[2] == 5.0 / (5.0 + 1e-6) and c[3] == 5.0 / (50.0 + 1e-6) and c[4] == 0
    assert np.isnan(c[5])
    assert (optim_ref.clip_coefs(np.array([0.0, 50.0, np.nan]), 0.0) == 1).all()
    # a passed coefficient is used as it is
    r = adam_clip_step_ref([np.ones(3)], [np.full(3, 100.0)], [np.zeros(3)], [np.zeros(3)], [0], [0], [True],
                           5.0, 1e-3, coef=np.array([0.25]), **HYP)
    assert np.array_equal(r["g"][0], np.full(3, 25.0)) and r["step"][0] == 1


# ---------------------------------------------------------------------------------------------
# chunk tables
# ---------------------------------------------------------------------------------------------
SIZES = [1, 5, 16, 17, 8192, 8193, 2 * 8192 + 4, 40, 3 * 8192]
TSEG = [0, 0, 1, 1, 1, 2, 2, 0, 3]


def _table_properties(T, sizes, seg_of, active, chunk=8192, align=16):
    nseg = T["nseg"]
    cb, ce, cs, cp, s0 = T["chunk_beg"], T["chunk_end"], T["chunk_seg"], T["chunk_param"], T["seg_chunk0"]
    assert cb.dtype == np.int64 and ce.dtype == np.int64
    assert all(a.dtype == np.int32 for a in (cs, cp, s0, T["active_params"]))
    assert len(s0) == nseg + 1 and s0[0] == 0 and s0[-1] == len(cb) and (np.diff(s0) >= 0).all()
    assert list(T["active_params"]) == [i for i, a in enumerate(active) if a]
    off = T["offsets"]
    spans = sorted((off[i], off[i] + -(-sizes[i] // align) * align) for i in range(len(sizes)))
    assert all(o % align == 0 for o in off)
    assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1)), "slices overlap"
    assert T["total"] == max(e for _, e in spans)
    covered = {i: [] for i, a in enumerate(active) if a}
    for c in range(len(cb)):
        i = int(cp[c])
        assert active[i], "an inactive parameter is listed"
        assert cs[c] == seg_of[i]
        assert s0[cs[c]] <= c < s0[cs[c] + 1], "a segment's chunks are not contiguous"
        assert cb[c] % align == 0 and (ce[c] - cb[c]) % 4 == 0 and 0 < ce[c] - cb[c] <= chunk
        assert off[i] <= cb[c] and ce[c] <= off[i] + -(-sizes[i] // align) * align, "a chunk straddles a parameter"
        covered[i].append((int(cb[c]), int(ce[c])))
    for i, spans_i in covered.items():      # each active padded slice exactly once, in order
        assert spans_i[0][0] == off[i] and spans_i[-1][1] == off[i] + -(-sizes[i] // align) * align
        assert all(spans_i[k][1] == spans_i[k + 1][0] for k in range(len(spans_i) - 1))
        assert len(spans_i) == -(-sizes[i] // chunk)


@pytest.mark.parametrize("inactive", [(), (0, 4), (5, 6), (2, 3, 4), tuple(range(9))])
def test_chunk_tables_follow_the_header(inactive):
    active = [i not in inactive for i in range(len(SIZES))]
    T = chunk_tables(SIZES, TSEG, active, nseg=5)         # segment 4 has no parameter at all
    _table_properties(T, SIZES, TSEG, active)
    assert T["seg_chunk0"][4] == T["seg_chunk0"][5]
    if len(inactive) == len(SIZES):
        assert len(T["chunk_beg"]) == 0 and (T["seg_chunk0"] == 0).all() and len(T["active_params"]) == 0


def test_chunk_tables_small_chunk_and_offsets():
    sizes, seg_of, active = [7, 100, 33], [1, 0, 1], [True, True, True]
    T = chunk_tables(sizes, seg_of, active, chunk=32, align=16, offsets=[160, 0, 112])
    _table_properties(T, sizes, seg_of, active, chunk=32)
    assert list(T["chunk_param"]) == [1, 1, 1, 1, 0, 2, 2] and list(T["seg_chunk0"]) == [0, 4, 7]
    assert list(T["chunk_beg"]) == [0, 32, 64, 96, 160, 112, 144] and T["total"] == 176


def _flat_adam_tables(opt):
    n = opt._nchunks
    return dict(chunk_beg=opt._cbeg[:n].numpy(), chunk_end=opt._cend[:n].numpy(), chunk_seg=opt._cseg[:n].numpy(),
                chunk_param=opt._cpar[:n].numpy(), seg_chunk0=opt._seg0.numpy(),
                active_params=opt._act[:opt._nact].numpy())


@pytest.mark.parametrize("first_inactive", [(), (1, 5), tuple(range(9))])
def test_flat_adam_builds_the_same_tables(first_inactive):
    """FlatAdam on CPU tensors: its layout satisfies the contract (parameters without a gradient at
    the first step lie behind the others) and, for that layout, _set_active lists what
    chunk_tables lists; again after the set of parameters with a gradient has changed."""
    from ured_hip.optim import ALIGN, CHUNK, FlatAdam
    assert (CHUNK, ALIGN) == (optim_ref.CHUNK, optim_ref.ALIGN)
    params = [torch.nn.Parameter(torch.randn(s)) for s in SIZES]
    segs = [[p for p, s in zip(params, TSEG) if s == k] for k in range(5)]
    order = [p for seg in segs for p in seg]              # FlatAdam numbers parameters segment by segment
    sizes = [p.numel() for p in order]
    seg_of = [k for k, seg in enumerate(segs) for _ in seg]
    opt = FlatAdam(params, segs, lr=1e-3, weight_decay=5e-4)
    for sets in (first_inactive, (0, 4), (), (2, 3, 4), tuple(range(9))):
        for i, p in enumerate(order):
            p.grad = None if i in sets else torch.zeros_like(p)
        active = list(opt.prepare())
        assert active == [i not in sets for i in range(len(order))]
        assert all(a is b for a, b in zip(opt.params_all, order))
        T = chunk_tables(sizes, seg_of, active, offsets=opt._off, nseg=5)
        _table_properties(T, sizes, seg_of, active)
        assert T["total"] == opt.flat_param.numel() == opt.flat_grad.numel() == opt.exp_avg.numel()
        got = _flat_adam_tables(opt)
        for key, val in got.items():
            assert val.dtype == T[key].dtype and np.array_equal(val, T[key]), key
    first = [i for i in range(len(order)) if i not in first_inactive]
    if first and first_inactive:
        assert max(opt._off[i] for i in first) < min(opt._off[i] for i in first_inactive)
    if not first_inactive:                                # everything active at first: index order
        assert opt._off == chunk_tables(sizes, seg_of, [True] * len(sizes))["offsets"]
