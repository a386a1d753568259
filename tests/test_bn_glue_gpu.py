"""The BatchNorm / max-pool glue kernels between the GEMM launches (csrc/mlp.hip): ured_bn_fwd_finalize,
ured_bn_bwd_finalize, ured_bn_bwd_apply (float4 and scalar kernels), ured_pool_finalize, ured_pool_rows
and ured_bn_act, each against float64 (tests/bn_ref.py) recomputed from the SAME device inputs
(the partials a ured_gemm launch left, or hand-built ones), so the bounds are rounding only:

  * finalize outputs are an fp64 result rounded to fp32 followed by at most three fp32
    operations: |got - ref| <= 4 * 2^-24 * (sum of |terms|) per element, the reference evaluated
    in double on the fp32 values the kernel itself rounded to (its mean / invstd outputs);
  * bn_bwd_apply: |dY - ref| <= 4 * 2^-24 * (|a g| + |w b (p - mu)| + |w c|) from the same fp32
    coefficients, column sums within 127 * 2^-24 * sum |dY| per block column;
  * pooled values and ured_bn_act within 1 fp32 ulp of the double evaluation; winners exact.

The forward statistics are also compared with bn_ref.bn_train_stats of the stored rows at 1e-5 of
the maximum, as the existing tests do.

Whole backward chain (EPI_BNBWD -> bn_bwd_finalize -> bn_bwd_apply vs bn_ref.bn_bwd_act): the
tolerance is measured, not chosen: the same formulas in plain fp32 torch on the CPU against float64
on the test's inputs give the fp32 yardstick; the kernels (another summation order) get 4x that,
with a floor of 1e-6 of the tensor's maximum, and 4x must stay below 1e-4 of the maximum. Measured
fp32 errors relative to the tensor's maximum, over the 24 cases (M 300 / 512, N 64 / 132, three
activation orders, with and without row weights):
    dgamma 1.1e-7 .. 2.2e-7    dbeta 9.0e-8 .. 3.2e-7    dY 9.1e-8 .. 2.4e-7
so 4x is 4e-7 .. 1.3e-6 and the kernels are held to 1e-6 .. 1.3e-6 of the maximum (the floor in
most cases)."""
import pytest
import torch

import bn_ref
from bn_ref import U32, f64

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))       # what the kernels see
MOM32 = float(torch.tensor(MOM, dtype=torch.float32))
SLACK = 1e-13       # float64 noise of the reference itself, relative to the terms


@pytest.fixture(scope="module")
def K(dev):
    from ured_hip import kernels
    return kernels


def _weights(M, group_rows, dev):
    """Row multiplicities [1, 3, 2, 1, 3, 2, ...] per group of group_rows rows."""
    G = (M + group_rows - 1) // group_rows
    return torch.tensor([1.0, 3.0, 2.0] * ((G + 2) // 3))[:G].to(dev)


def _within(got, ref, bound, name):
    got, ref, bound = f64(got), f64(ref), f64(bound)
    over = (got - ref).abs() - bound * (1 + SLACK) - 1e-300
    assert (over <= 0).all(), f"{name}: |got - ref| exceeds the rounding bound by {over.max().item():.3e} " \
                              f"(bound {bound.flatten()[over.argmax()].item():.3e})"


_FWD = {}


def _fwd_launch(K, dev, M, N):
    """EPI_FWD launch (K = 8) -> stored Y [M][N] and its block partials, cached per shape (read only)."""
    if (M, N) not in _FWD:
        g = torch.Generator().manual_seed(M + N)
        X = torch.randn(M, 8, generator=g)
        W = torch.randn(N, 8, generator=g) * 0.5
        b = torch.randn(N, generator=g) + 0.5          # columns with a clear mean: no cancellation in the merge
        Y = torch.empty(M, N, device=dev)
        ws = torch.empty(2, N, K.nblocks(M), device=dev)
        K.gemm(M, N, 8, X.to(dev), 8, W.to(dev), 8, Y, N, epi=K.EPI_FWD, bias=b.to(dev), stat_ws=ws)
        _FWD[(M, N)] = (Y, ws)
    return _FWD[(M, N)]


# ------------------------------------------------------------------ bn_fwd_finalize

@pytest.mark.parametrize("group_rows", [0, 128, 256], ids=["unweighted", "rw128", "rw256"])
@pytest.mark.parametrize("N", [3, 64])
@pytest.mark.parametrize("M", [1, 127, 129, 300, 33000])      # 33000 rows = 258 blocks: the 256-thread loop wraps
def test_bn_fwd_finalize(K, dev, M, N, group_rows):
    Y, ws = _fwd_launch(K, dev, M, N)
    gw = _weights(M, group_rows, dev) if group_rows else None
    rw = K.RowWeights(gw, group_rows) if group_rows else None
    Mw, mean64, m2, mean_terms = bn_ref.merge_partials(ws, M, gw, group_rows)
    rows = bn_ref.bn_train_stats(Y, bn_ref.row_weights(gw, group_rows, M), EPS32, MOM32)
    assert Mw.item() == rows["count"].item()
    g = torch.Generator().manual_seed(5)
    for affine in (True, False):
        for running in (True, False):
            gamma = (torch.randn(N, generator=g)).to(dev) if affine else None
            beta = torch.randn(N, generator=g).to(dev) if affine else None
            rm0, rv0 = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5
            rm, rv = (rm0.to(dev), rv0.to(dev)) if running else (None, None)
            nbt = torch.tensor([41], dtype=torch.int64, device=dev)
            st = K.bn_fwd_finalize(ws, M, N, gamma, beta, EPS, MOM, rm, rv, rw=rw, num_batches_tracked=nbt)
            assert nbt.item() == 42
            name = f"M={M} N={N} affine={affine} running={running}"
            is64 = 1.0 / torch.sqrt(m2 / Mw + EPS32)
            _within(st.mean, mean64, 4 * U32 * mean_terms, name + " mean")
            _within(st.invstd, is64, 4 * U32 * is64, name + " invstd")
            mf, isf = f64(st.mean), f64(st.invstd)          # the fp32 values the kernel continues from
            ga = f64(gamma) if affine else torch.ones(N, dtype=torch.float64)
            be = f64(beta) if affine else torch.zeros(N, dtype=torch.float64)
            sc = ga * isf
            _within(st.scale, sc, 4 * U32 * sc.abs(), name + " scale")
            _within(st.shift, be - mf * sc, 4 * U32 * (be.abs() + (mf * sc).abs()), name + " shift")
            if running:
                uv = (m2 / (Mw - 1.0) if Mw > 1 else m2).float().double()     # M = 1: the Mw > 1 guard
                t1 = (1.0 - MOM32) * f64(rm0)
                _within(rm, t1 + MOM32 * mf, 4 * U32 * (t1.abs() + (MOM32 * mf).abs()), name + " running_mean")
                t1 = (1.0 - MOM32) * f64(rv0)
                _within(rv, t1 + MOM32 * uv, 4 * U32 * (t1.abs() + (MOM32 * uv).abs()), name + " running_var")
            # and against the stored rows themselves (fp32 block partials in between): 1e-5 of max
            want = bn_ref.bn_outputs(rows["count"], rows["mean"], rows["m2"], EPS32, MOM32, rm0 if running else None,
                                     rv0 if running else None, gamma, beta)
            pairs = [("mean", st.mean), ("invstd", st.invstd), ("scale", st.scale), ("shift", st.shift)]
            if running:
                pairs += [("running_mean", rm), ("running_var", rv)]
            for key, got in pairs:
                err = (f64(got) - want[key]).abs().max().item()
                assert err <= 1e-5 * max(want[key].abs().max().item(), 1e-6), f"{name} {key} vs rows: {err:.3e}"


# ------------------------------------------------------------------ bn_bwd_finalize

@pytest.mark.parametrize("group_rows", [0, 128, 256], ids=["unweighted", "rw128", "rw256"])
@pytest.mark.parametrize("N", [3, 64])
@pytest.mark.parametrize("M", [1, 127, 129, 300, 33000])
def test_bn_bwd_finalize(K, dev, M, N, group_rows):
    from ured_hip import _lib
    g = torch.Generator().manual_seed(M + N + group_rows)
    ws = torch.randn(2, N, K.nblocks(M), generator=g).to(dev)        # hand-built partials
    invstd = (torch.rand(N, generator=g) + 0.5).to(dev)
    gw = _weights(M, group_rows, dev) if group_rows else None
    rw = K.RowWeights(gw, group_rows) if group_rows else None
    for affine in (True, False):
        gamma = torch.randn(N, generator=g).to(dev) if affine else None
        val, mag = bn_ref.bwd_finalize_terms(ws, M, gamma, invstd, gw, group_rows)
        dgamma, dbeta = torch.full((N,), 9.0, device=dev), torch.full((N,), -9.0, device=dev)
        ca, cb, cc = K.bn_bwd_finalize(ws, M, N, gamma, invstd, dgamma, dbeta, rw=rw)
        for key, got in (("dgamma", dgamma), ("dbeta", dbeta), ("ca", ca), ("cb", cb), ("cc", cc)):
            _within(got, val[key], 4 * U32 * mag[key], f"M={M} N={N} affine={affine} {key}")
        # accumulate = 1 (the wrapper hard-codes 0): prior contents + the sums, one more rounding
        pg, pb = torch.randn(N, generator=g), torch.randn(N, generator=g)
        dgamma, dbeta = pg.to(dev), pb.to(dev)
        c2 = [torch.empty(N, device=dev) for _ in range(3)]
        gwp, grows = (None, 0) if rw is None else (rw.w.data_ptr(), rw.group_rows)
        _lib.call("ured_bn_bwd_finalize", ws.data_ptr(), M, N, None if gamma is None else gamma.data_ptr(),
                  invstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), 1, c2[0].data_ptr(), c2[1].data_ptr(),
                  c2[2].data_ptr(), gwp, grows, _lib.stream_of(ws))
        _within(dgamma, f64(pg) + val["dgamma"], 4 * U32 * (f64(pg).abs() + mag["dgamma"]), "accumulated dgamma")
        _within(dbeta, f64(pb) + val["dbeta"], 4 * U32 * (f64(pb).abs() + mag["dbeta"]), "accumulated dbeta")
        assert torch.equal(c2[0], ca) and torch.equal(c2[1], cb) and torch.equal(c2[2], cc)


# ------------------------------------------------------------------ bn_bwd_apply

def _apply(K, G, Y, dY, M, N, ld, res, mean, coefs, cs, gw, group_rows):
    from ured_hip import _lib
    _lib.call("ured_bn_bwd_apply", G.data_ptr(), Y.data_ptr(), M, N, ld, int(res), mean.data_ptr(),
              coefs[0].data_ptr(), coefs[1].data_ptr(), coefs[2].data_ptr(), dY.data_ptr(),
              None if cs is None else cs.data_ptr(), None if gw is None else gw.data_ptr(), group_rows,
              _lib.stream_of(Y))


def _apply_inputs(M, N, res, seed):
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(M, N, generator=g)
    Y = torch.randn(M, N, generator=g)
    if res:         # Conv -> ReLU -> BN: no gradient where y <= 0, at y = +0 and -0 too
        Y.view(-1)[::7] = 0.0
        Y.view(-1)[3::11] = -0.0
    mean = torch.randn(N, generator=g) * 0.3
    coefs = [torch.randn(N, generator=g), torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g) * 0.1]
    return G, Y, mean, coefs


def _apply_ref(G, Y, res, mean, coefs, w_rows):
    """-> float64 dY from the fp32 inputs and the bound 4u (|a g| + |w b (p - mu)| + |w c|)."""
    g, y, mu = f64(G), f64(Y), f64(mean)
    a, b, c = (f64(x) for x in coefs)
    w = torch.ones(y.shape[0], 1, dtype=torch.float64) if w_rows is None else w_rows[:, None]
    p = y.clamp_min(0) if res else y
    t1, t2, t3 = a * g, w * b * (p - mu), w * c
    v, mag = t1 + t2 + t3, t1.abs() + t2.abs() + t3.abs()
    if res:
        v = torch.where(y > 0, v, torch.zeros_like(v))
        mag = torch.where(y > 0, mag, torch.zeros_like(mag))       # exactly 0 where masked
    return v, 4 * U32 * mag


def _colsum_check(K, cs, dY, M, name):
    d = f64(dY)
    for blk in range(K.nblocks(M)):
        rows = d[blk * 128:(blk + 1) * 128]
        _within(cs[blk], rows.sum(0), 127 * U32 * rows.abs().sum(0), f"{name} colsum block {blk}")


# (M, N, kernel): float4 needs N % 4 == 0 and 16-byte aligned bases
APPLY_SHAPES = [(1, 64, "float4"), (127, 64, "float4"), (300, 132, "float4"), (300, 70, "scalar"), (300, 3, "scalar")]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "rw128"])
@pytest.mark.parametrize("res", [0, 1], ids=["enc", "res"])
@pytest.mark.parametrize("M,N,kernel", APPLY_SHAPES, ids=[f"{s[0]}x{s[1]}-{s[2]}" for s in APPLY_SHAPES])
def test_bn_bwd_apply(K, dev, M, N, kernel, res, weighted):
    G, Y, mean, coefs = _apply_inputs(M, N, res, 100 * M + N + res)
    gw = _weights(M, 128, dev) if weighted else None
    w_rows = bn_ref.row_weights(gw, 128, M)
    ref, bound = _apply_ref(G, Y, res, mean, coefs, w_rows)
    Gd, Yd, md, cd = G.to(dev), Y.to(dev), mean.to(dev), [c.to(dev) for c in coefs]
    name = f"{M}x{N} {kernel} res={res} weighted={weighted}"
    outs = []
    for want_colsum in (True, False):
        dY = torch.full((M, N), float("nan"), device=dev)
        cs = torch.full((K.nblocks(M), N), float("nan"), device=dev) if want_colsum else None
        _apply(K, Gd, Yd, dY, M, N, N, res, md, cd, cs, gw, 128)
        _within(dY, ref, bound, name + " dY")
        if res:
            assert (dY.cpu()[~(Y > 0)] == 0).all(), "gradient where y <= 0"
        if want_colsum:
            _colsum_check(K, cs, dY, M, name)
        outs.append(dY)
    assert torch.equal(outs[0], outs[1])
    # the wrapper the training step uses
    dY2, cs2 = K.bn_bwd_apply(Gd, Yd, res, md, cd, want_colsum=True, rw=K.RowWeights(gw, 128) if weighted else None)
    assert torch.equal(dY2, outs[0])
    if kernel == "float4" and M > 1:
        # G, Y, dY carved from flat buffers at a 1-element offset: 4-byte aligned only -> the scalar
        # kernel; the same fma chain per element, so dY is bitwise the float4 kernel's
        flat = [torch.zeros(M * N + 1, device=dev) for _ in range(3)]
        Go, Yo, dYo = (f[1:].view(M, N) for f in flat)
        Go.copy_(Gd)
        Yo.copy_(Yd)
        assert Go.data_ptr() % 16 == 4
        cs = torch.full((K.nblocks(M), N), float("nan"), device=dev)
        _apply(K, Go, Yo, dYo, M, N, N, res, md, cd, cs, gw, 128)
        assert torch.equal(dYo, outs[0]), "scalar kernel differs from the float4 kernel"
        _colsum_check(K, cs, dYo, M, name + " (scalar kernel)")


# ------------------------------------------------------------------ the whole backward chain

def _chain_fp32(dYin, W, y, act, mask, mean, invstd, gamma, w_rows):
    """bn_ref.bn_bwd_act's formulas in plain fp32 torch (the yardstick); the ENC mask is given."""
    dh = dYin @ W
    if act == bn_ref.ACT_ENC:
        g, p = torch.where(mask, dh, torch.zeros_like(dh)), y
    elif act == bn_ref.ACT_RES:
        g, p = dh, y.clamp_min(0)
    else:
        g, p = dh, y
    xh = (p - mean) * invstd
    db, dg = g.sum(0), (g * xh).sum(0)
    w = torch.ones(y.shape[0], dtype=torch.float32) if w_rows is None else w_rows.float()
    Mw = w.sum()
    k = gamma * invstd
    dp = k * g + w[:, None] * ((-k * invstd * dg / Mw) * (p - mean) + (-k * db / Mw))
    if act == bn_ref.ACT_RES:
        dp = torch.where(y > 0, dp, torch.zeros_like(dp))
    return {"dgamma": dg, "dbeta": db, "dY": dp}


def _chain_case(M, N, act, weighted):
    """Inputs of one chain case (CPU), the float64 reference and the fp32-torch yardstick."""
    Kd = 8
    g = torch.Generator().manual_seed(M + N + act)
    dYin = torch.randn(M, Kd, generator=g)
    W = torch.randn(Kd, N, generator=g) * Kd ** -0.5
    y = torch.randn(M, N, generator=g) * 1.5 + 0.25
    gamma = (torch.rand(N, generator=g) + 0.5) * (torch.randint(0, 2, (N,), generator=g).float() * 2 - 1)   # both signs
    beta = torch.randn(N, generator=g) * 0.5
    gw = _weights(M, 128, "cpu") if weighted else None
    w_rows = bn_ref.row_weights(gw, 128, M)
    p = y.clamp_min(0) if act == bn_ref.ACT_RES else y
    st = bn_ref.bn_train_stats(p, w_rows, EPS32, MOM32, gamma=gamma, beta=beta)
    # the layer's statistics as the device holds them (fp32); the reference starts from these
    mean, invstd, scale, shift = (st[k].float() for k in ("mean", "invstd", "scale", "shift"))
    dh = dYin.double() @ W.double()
    ref = bn_ref.bn_bwd_act(dh, y, act, mean, invstd, scale, shift, gamma, w_rows)
    # y*scale+shift of fp32 values is exact in double up to one rounding that keeps its sign: the
    # float64 mask is the kernel's fp32 fma mask
    mask = y.double() * scale.double() + shift.double() > 0
    y32 = _chain_fp32(dYin, W, y, act, mask, mean, invstd, gamma, w_rows)
    return dYin, W, y, gamma, gw, (mean, invstd, scale, shift), ref, y32


CHAIN_SHAPES = [(300, 64), (300, 132), (512, 64), (512, 132)]
CHAIN_ACTS = [bn_ref.ACT_ENC, bn_ref.ACT_RES, bn_ref.ACT_BN]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "rw128"])
@pytest.mark.parametrize("act", CHAIN_ACTS, ids=["enc", "res", "bn"])
@pytest.mark.parametrize("M,N", CHAIN_SHAPES)
def test_bn_backward_chain(K, dev, M, N, act, weighted):
    Kd = 8
    dYin, W, y, gamma, gw, (mean, invstd, scale, shift), ref, y32 = _chain_case(M, N, act, weighted)
    gw = None if gw is None else gw.to(dev)

    G = torch.empty(M, N, device=dev)
    ws = torch.empty(2, N, K.nblocks(M), device=dev)
    bn = K.BNState(mean.to(dev), invstd.to(dev), scale.to(dev), shift.to(dev))
    yd = y.to(dev)
    K.gemm(M, N, Kd, dYin.to(dev), Kd, W.to(dev), N, G, N, b_kmajor=True, epi=K.EPI_BNBWD, Yp=yd, ldy=N, bn=bn,
           bwd_res=act, bwd_ws=ws)
    rw = K.RowWeights(gw, 128) if weighted else None
    dgamma, dbeta = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    coefs = K.bn_bwd_finalize(ws, M, N, gamma.to(dev), bn.invstd, dgamma, dbeta, rw=rw)
    dY, _ = K.bn_bwd_apply(G, yd, act == bn_ref.ACT_RES, bn.mean, coefs, rw=rw)
    for key, got in (("dgamma", dgamma), ("dbeta", dbeta), ("dY", dY)):
        top = ref[key].abs().max().item()
        e32 = (y32[key].double() - ref[key]).abs().max().item()
        err = (f64(got) - ref[key]).abs().max().item()
        print(f"chain M={M} N={N} act={act} weighted={weighted} {key}: fp32 torch {e32 / top:.2e} kernels {err / top:.2e} of max")
        assert 4 * e32 <= 1e-4 * top, f"{key}: ill-conditioned inputs (fp32 torch is off by {e32 / top:.2e} of max)"
        assert err <= max(4 * e32, 1e-6 * top), f"{key}: {err:.3e} > max(4 * {e32:.3e}, 1e-6 * {top:.3e})"


# ------------------------------------------------------------------ pool_finalize / pool_rows

TIE_ROWS = [10, 130, 134, 138, 162, 200, 300, 400]     # copies of one row of A -> bitwise equal rows of Y


@pytest.fixture(scope="module")
def pooled_y(K, dev):
    """EPI_FWD with pool_ws on 512 rows, N = 70 (a partial column tile), with forced ties."""
    M, N, Kd = 512, 70, 32
    g = torch.Generator().manual_seed(70)
    X = torch.randn(M, Kd, generator=g)
    X[TIE_ROWS] = 8.0 * X[TIE_ROWS[0]]          # the copied row is the column max or min in most columns
    W = torch.randn(N, Kd, generator=g) * Kd ** -0.5
    Y = torch.empty(M, N, device=dev)
    ws = torch.empty(2, N, K.nblocks(M), device=dev)
    pw = torch.empty(K.nblocks(M), 4, N, device=dev)
    K.gemm(M, N, Kd, X.to(dev), Kd, W.to(dev), Kd, Y, N, epi=K.EPI_FWD, stat_ws=ws, pool_ws=pw, group_rows=128)
    scale = torch.randn(N, generator=g)
    scale[3] = 0.0                              # exact 0: every row ties
    scale[5] = -0.0
    shift = torch.randn(N, generator=g)
    assert (scale < 0).sum() > 5 and (scale > 0).sum() > 5
    Yc = Y.cpu()
    assert all(torch.equal(Yc[10], Yc[r]) for r in TIE_ROWS[1:6])
    return Y, Yc, pw, scale, shift


def _pool_check(pooled, argidx, Yc, group_rows, scale, shift, relu, name):
    want, widx, _ = bn_ref.pool_ref(Yc, group_rows, scale, shift, relu)
    idx = argidx.cpu().long()
    nz = scale != 0
    assert torch.equal(idx[:, nz], widx[:, nz]), f"{name}: winners"
    lo = (torch.arange(idx.shape[0]) * group_rows)[:, None]
    assert ((idx >= lo) & (idx < lo + group_rows)).all(), f"{name}: winner outside its group"
    # scale = 0: the value is shift whatever the winner
    r32 = want.float().double()
    assert ((f64(pooled) - r32).abs() <= bn_ref.ulp32(r32)).all(), f"{name}: pooled value"
    if relu:
        assert (pooled >= 0).all()


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_pool_finalize_and_rows(K, dev, pooled_y, relu):
    Y, Yc, pw, scale, shift = pooled_y
    M, N = Y.shape
    sd, hd = scale.to(dev), shift.to(dev)
    for gr in (128, 256):       # 128-aligned groups: both kernels, the same answer bit for bit
        pf, af = K.pool_finalize(pw, M, N, gr, sd, hd, relu=relu)
        pr, ar = K.pool_rows(Y, gr, sd, hd, relu=relu)
        _pool_check(pf, af, Yc, gr, scale, shift, relu, f"pool_finalize group_rows={gr}")
        _pool_check(pr, ar, Yc, gr, scale, shift, relu, f"pool_rows group_rows={gr}")
        assert torch.equal(pf, pr) and torch.equal(af, ar), f"pool_finalize != pool_rows at group_rows={gr}"
    # the forced ties decide winners: group 0 of 256 rows holds the copies 10, 130 .. 200
    _, widx, _ = bn_ref.pool_ref(Yc, 256, scale, shift, relu)
    assert (widx[0] == 10).sum().item() >= N // 8
    for gr in (5, 100):         # pool_rows alone, any group size (500 rows)
        Ys = Y[:500]
        pr, ar = K.pool_rows(Ys, gr, sd, hd, relu=relu)
        _pool_check(pr, ar, Yc[:500], gr, scale, shift, relu, f"pool_rows group_rows={gr}")


# ------------------------------------------------------------------ bn_act

@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("M,N", [(300, 64), (7, 6)])
def test_bn_act(K, dev, M, N, relu):
    g = torch.Generator().manual_seed(M + N)
    Y = torch.randn(M, N, generator=g)
    scale, shift = torch.randn(N, generator=g), torch.randn(N, generator=g)
    st = K.BNState(None, None, scale.to(dev), shift.to(dev))
    ref = Y.double() * scale.double() + shift.double()
    if relu:
        ref = ref.clamp_min(0)
    r32 = ref.float().double()
    outs = []
    for pad in (4, 1):      # row pitch N + 4: float4 kernel when N % 4 == 0; N + 1: the scalar kernel
        buf = torch.zeros(M, N + pad, device=dev)
        view = buf[:, :N]
        view.copy_(Y.to(dev))
        assert view.stride(0) == N + pad
        out = K.bn_act(view, st, relu=relu)
        assert ((f64(out) - r32).abs() <= bn_ref.ulp32(r32)).all(), f"bn_act pitch N+{pad}"
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "float4 and scalar bn_act differ"
