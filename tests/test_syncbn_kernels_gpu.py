"""The four SyncBN kernels (csrc/syncbn.hip: ured_bn_stats, ured_bn_finalize_stats, ured_bn_bwd_sums,
ured_bn_bwd_finalize_sums) in ONE process: a batch is cut into "ranks", each rank's kernels run on
its own rows, and the cross-rank exchange is done by the test itself in float64 (Chan's merge for
the forward, a plain sum for the backward), so no process group is needed. ured_hip.syncbn is
imported for the registered signatures only; the entries are called through _lib.call.

Two splits of the rows:
  * 300 + 129 + 1 rows (rank 0 with row weights [1, 3, 2] per 128-row group, a partial last
    block on every rank, a one-row rank): each rank's (count, mean, M2) against float64 of its
    expanded rows (count exact, mean and M2 to 1e-6 relative; the columns have a clear mean),
    and the finalized outputs against bn_ref.bn_train_stats of the whole expanded batch at 1e-5
    of the maximum;
  * 256 + 384 + 45 rows (rank 0 weighted): every rank boundary falls on a 128-row block, so the
    ranks' partials laid side by side ARE the partials of the concatenated batch and
    ured_bn_fwd_finalize / ured_bn_bwd_finalize on them must give the same outputs as the split
    kernels within the rounding bound 4 * 2^-24 * (sum of |terms|) (with other sizes the blocks of
    the concatenated batch would be other blocks, and the comparison one of fp32 partials).
A single rank through the split pair must reproduce the fused finalizes within one fp32
rounding of the terms (2^-23 * sum of |terms|): the identity the 2-process test relies on."""
import pytest
import torch

import bn_ref
from bn_ref import U32, f64

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
MOM32 = float(torch.tensor(MOM, dtype=torch.float32))
KD = 8


@pytest.fixture(scope="module")
def K(dev):
    from ured_hip import kernels, syncbn       # noqa: F401  (syncbn registers the entry points' signatures)
    return kernels


def _call(name, *args):
    from ured_hip import _lib
    _lib.call(name, *args)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    from ured_hip import _lib
    return _lib.stream_of(t)


def _within(got, ref, bound, name):
    over = (f64(got) - f64(ref)).abs() - f64(bound) * (1 + 1e-13) - 1e-300
    assert (over <= 0).all(), f"{name}: over the rounding bound by {over.max().item():.3e}"


class Rank:
    """One rank's rows: the EPI_FWD launch (Y, forward partials) and its row weights."""

    def __init__(self, K, dev, M, N, weighted, seed):
        g = torch.Generator().manual_seed(seed)
        X = torch.randn(M, KD, generator=g)
        W = torch.randn(N, KD, generator=g) * 0.25
        b = (torch.rand(N, generator=g) + 1.0) * (torch.randint(0, 2, (N,), generator=g).float() * 2 - 1)   # |mean| >= ~1
        self.M, self.N = M, N
        self.Y = torch.empty(M, N, device=dev)
        self.ws = torch.empty(2, N, K.nblocks(M), device=dev)
        K.gemm(M, N, KD, X.to(dev), KD, W.to(dev), KD, self.Y, N, epi=K.EPI_FWD, bias=b.to(dev), stat_ws=self.ws)
        G = (M + 127) // 128
        self.gw = torch.tensor([1.0, 3.0, 2.0] * ((G + 2) // 3))[:G].to(dev) if weighted else None
        self.grows = 128 if weighted else 0
        self.w_rows = bn_ref.row_weights(self.gw, 128, M) if weighted else torch.ones(M, dtype=torch.float64)
        self.block_w = torch.ones(G) if self.gw is None else self.gw.cpu()

    def stats(self):
        out = torch.full((3, self.N), float("nan"), dtype=torch.float64, device=self.Y.device)
        _call("ured_bn_stats", _p(self.ws), self.M, self.N, _p(self.gw), self.grows, _p(out), _stream(self.ws))
        return out


def _ranks(K, dev, sizes, N):
    return [Rank(K, dev, M, N, weighted=(i == 0), seed=31 * i + M + N) for i, M in enumerate(sizes)]


def _chan(stats):
    """float64 merge of per-rank [3][N] (count, mean, M2) in rank order."""
    st = torch.stack([f64(s) for s in stats])
    c, mu, m2 = st[:, 0], st[:, 1], st[:, 2]
    C = c.sum(0)
    mean = (c * mu).sum(0) / C
    return torch.stack([C, mean, (m2 + c * (mu - mean) ** 2).sum(0)])


def _finalize_stats(dev, glob, N, gamma, beta, rm, rv, nbt):
    out = [torch.full((N,), float("nan"), device=dev) for _ in range(4)]
    gd = glob.to(dev)
    _call("ured_bn_finalize_stats", _p(gd), N, _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv), *[_p(o) for o in out],
          _p(nbt), _stream(gd))
    return out


def _params(N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = torch.randn(N, generator=g), torch.randn(N, generator=g)
    rm, rv = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5
    return gamma.to(dev), beta.to(dev), rm, rv


NAMES = ("mean", "invstd", "scale", "shift")


@pytest.mark.parametrize("N", [64, 6])
def test_forward_split_vs_float64(K, dev, N):
    ranks = _ranks(K, dev, [300, 129, 1], N)
    stats = [r.stats() for r in ranks]
    for i, (r, s) in enumerate(zip(ranks, stats)):
        want = bn_ref.bn_train_stats(r.Y, r.w_rows)
        s = s.cpu()
        assert torch.equal(s[0], torch.full((N,), want["count"].item(), dtype=torch.float64)), f"rank {i} count"
        assert ((s[1] - want["mean"]).abs() <= 1e-6 * want["mean"].abs()).all(), f"rank {i} mean"
        assert ((s[2] - want["m2"]).abs() <= 1e-6 * want["m2"].abs()).all(), f"rank {i} M2"
    gamma, beta, rm0, rv0 = _params(N, dev, N)
    rm, rv = rm0.to(dev), rv0.to(dev)
    nbt = torch.tensor([7], dtype=torch.int64, device=dev)
    got = _finalize_stats(dev, _chan(stats), N, gamma, beta, rm, rv, nbt)
    assert nbt.item() == 8
    want = bn_ref.bn_train_stats(torch.cat([r.Y for r in ranks]), torch.cat([r.w_rows for r in ranks]), EPS32, MOM32,
                                 rm0, rv0, gamma, beta)
    for key, t in list(zip(NAMES, got)) + [("running_mean", rm), ("running_var", rv)]:
        err = (f64(t) - want[key]).abs().max().item()
        assert err <= 1e-5 * want[key].abs().max().item(), f"{key}: {err:.3e}"


@pytest.mark.parametrize("N", [64, 6])
def test_forward_split_vs_fused_on_concatenated_batch(K, dev, N):
    ranks = _ranks(K, dev, [256, 384, 45], N)
    gamma, beta, rm0, rv0 = _params(N, dev, N + 1)
    rm, rv = rm0.to(dev), rv0.to(dev)
    nbt = torch.tensor([0], dtype=torch.int64, device=dev)
    got = _finalize_stats(dev, _chan([r.stats() for r in ranks]), N, gamma, beta, rm, rv, nbt)
    # block-aligned ranks: their partials side by side are the concatenated batch's partials
    M = sum(r.M for r in ranks)
    ws = torch.cat([r.ws for r in ranks], dim=2).contiguous()
    gw = torch.cat([r.block_w for r in ranks]).to(dev)
    rm2, rv2 = rm0.to(dev), rv0.to(dev)
    nbt2 = torch.tensor([0], dtype=torch.int64, device=dev)
    st = K.bn_fwd_finalize(ws, M, N, gamma, beta, EPS, MOM, rm2, rv2, rw=K.RowWeights(gw, 128), num_batches_tracked=nbt2)
    assert nbt.item() == 1 and nbt2.item() == 1
    Mw, mean, m2, mean_terms = bn_ref.merge_partials(ws, M, gw, 128)
    out = bn_ref.bn_outputs(Mw, mean, m2, EPS32, MOM32, rm0, rv0, gamma, beta)
    mag = bn_ref.fwd_output_sizes(out, mean_terms, MOM32, rm0, rv0, gamma, beta)
    fused = dict(zip(NAMES, (st.mean, st.invstd, st.scale, st.shift)), running_mean=rm2, running_var=rv2)
    for key, t in list(zip(NAMES, got)) + [("running_mean", rm), ("running_var", rv)]:
        _within(t, fused[key], 4 * U32 * mag[key], f"split vs fused {key}")
        _within(t, out[key], 5 * U32 * mag[key], f"split vs float64 {key}")      # five roundings from pure float64


def _bwd_rank(K, dev, r, bn, act, seed):
    """EPI_BNBWD on one rank's rows with the global statistics -> backward partials [2][N][blocks]."""
    g = torch.Generator().manual_seed(seed)
    dY = torch.randn(r.M, KD, generator=g)
    W = torch.randn(KD, r.N, generator=g) * KD ** -0.5
    G = torch.empty(r.M, r.N, device=dev)
    ws = torch.empty(2, r.N, K.nblocks(r.M), device=dev)
    K.gemm(r.M, r.N, KD, dY.to(dev), KD, W.to(dev), r.N, G, r.N, b_kmajor=True, epi=K.EPI_BNBWD, Yp=r.Y, ldy=r.N, bn=bn,
           bwd_res=act, bwd_ws=ws)
    return ws


def _bwd_sums(r, ws):
    out = torch.full((3, r.N), float("nan"), dtype=torch.float64, device=ws.device)
    _call("ured_bn_bwd_sums", _p(ws), r.M, r.N, _p(r.gw), r.grows, _p(out), _stream(ws))
    return out


def _finalize_sums(dev, local, glob, N, gamma, invstd, dgamma, dbeta, accumulate):
    co = [torch.full((N,), float("nan"), device=dev) for _ in range(3)]
    _call("ured_bn_bwd_finalize_sums", _p(local), _p(glob), N, _p(gamma), _p(invstd), _p(dgamma), _p(dbeta),
          int(accumulate), *[_p(c) for c in co], _stream(local))
    return co


@pytest.mark.parametrize("sizes", [[300, 129, 1], [256, 384, 45]], ids=["300+129+1", "256+384+45-block_aligned"])
@pytest.mark.parametrize("N", [64, 8])      # N % 4 == 0: k-major W of the dgrad GEMM
def test_backward_split(K, dev, N, sizes):
    ranks = _ranks(K, dev, sizes, N)
    gamma, beta, _, _ = _params(N, dev, N + 2)
    mean, invstd, scale, shift = _finalize_stats(dev, _chan([r.stats() for r in ranks]), N, gamma, beta, None, None, None)
    bn = K.BNState(mean, invstd, scale, shift)
    wss = [_bwd_rank(K, dev, r, bn, bn_ref.ACT_ENC, 5 + i) for i, r in enumerate(ranks)]
    sums = [_bwd_sums(r, ws) for r, ws in zip(ranks, wss)]
    for i, (r, ws, s) in enumerate(zip(ranks, wss, sums)):
        w, s = f64(ws), s.cpu()
        for q in (0, 1):
            assert ((s[q] - w[q].sum(1)).abs() <= 1e-12 * w[q].abs().sum(1)).all(), f"rank {i} sum {q}"
        assert torch.equal(s[2], torch.full((N,), r.w_rows.sum().item(), dtype=torch.float64)), f"rank {i} count"
    glob = torch.stack(sums).sum(0)          # the all-reduce
    aligned = all(r.M % 128 == 0 for r in ranks[:-1])
    if aligned:     # the fused finalize on the concatenated batch (see the module docstring)
        M = sum(r.M for r in ranks)
        ws_all = torch.cat(wss, dim=2).contiguous()
        gw = torch.cat([r.block_w for r in ranks]).to(dev)
        dg2, db2 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        fused = K.bn_bwd_finalize(ws_all, M, N, gamma, invstd, dg2, db2, rw=K.RowWeights(gw, 128))
        val, mag = bn_ref.bwd_finalize_terms(ws_all, M, gamma, invstd, gw, 128)
        assert val["count"].item() == glob[2, 0].item()
    for i, s in enumerate(sums):
        dgamma, dbeta = torch.full((N,), 5.0, device=dev), torch.full((N,), -5.0, device=dev)
        co = _finalize_sums(dev, s, glob, N, gamma, invstd, dgamma, dbeta, 0)
        # dgamma / dbeta are the rank's LOCAL sums (the gradient all-reduce averages them later)
        assert torch.equal(dgamma, s[1].float()) and torch.equal(dbeta, s[0].float()), f"rank {i} local sums"
        pg = torch.randn(N, generator=torch.Generator().manual_seed(i)).to(dev)
        dgamma, dbeta = pg.clone(), -pg
        co2 = _finalize_sums(dev, s, glob, N, gamma, invstd, dgamma, dbeta, 1)
        assert torch.equal(dgamma, pg + s[1].float()) and torch.equal(dbeta, -pg + s[0].float()), f"rank {i} accumulate"
        assert all(torch.equal(a, b) for a, b in zip(co, co2))
        if aligned:
            for key, a, b in zip(("ca", "cb", "cc"), co, fused):
                _within(a, b, 4 * U32 * mag[key], f"rank {i} {key} split vs fused")
                _within(a, val[key], 4 * U32 * mag[key], f"rank {i} {key} vs float64")


@pytest.mark.parametrize("M,weighted", [(300, True), (129, False), (1, False)])
def test_single_rank_reproduces_fused_finalizes(K, dev, M, weighted):
    """World size 1 through the split kernels = the fused kernels, within one fp32 rounding."""
    N = 64
    r = Rank(K, dev, M, N, weighted, seed=M)
    gamma, beta, rm0, rv0 = _params(N, dev, M)
    rm, rv = rm0.to(dev), rv0.to(dev)
    nbt = torch.tensor([3], dtype=torch.int64, device=dev)
    got = _finalize_stats(dev, r.stats().cpu(), N, gamma, beta, rm, rv, nbt)
    rm2, rv2 = rm0.to(dev), rv0.to(dev)
    rw = K.RowWeights(r.gw, 128) if weighted else None
    st = K.bn_fwd_finalize(r.ws, M, N, gamma, beta, EPS, MOM, rm2, rv2, rw=rw)
    assert nbt.item() == 4
    Mw, mean, m2, mean_terms = bn_ref.merge_partials(r.ws, M, r.gw, r.grows)
    out = bn_ref.bn_outputs(Mw, mean, m2, EPS32, MOM32, rm0, rv0, gamma, beta)
    mag = bn_ref.fwd_output_sizes(out, mean_terms, MOM32, rm0, rv0, gamma, beta)
    fused = dict(zip(NAMES, (st.mean, st.invstd, st.scale, st.shift)), running_mean=rm2, running_var=rv2)
    for key, t in list(zip(NAMES, got)) + [("running_mean", rm), ("running_var", rv)]:
        _within(t, fused[key], 2 * U32 * mag[key], f"forward {key}")
    bn = K.BNState(st.mean, st.invstd, st.scale, st.shift)
    ws = _bwd_rank(K, dev, r, bn, bn_ref.ACT_RES, 9)
    s = _bwd_sums(r, ws)
    dgamma, dbeta = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    co = _finalize_sums(dev, s, s, N, gamma, st.invstd, dgamma, dbeta, 0)
    dg2, db2 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    fused = K.bn_bwd_finalize(ws, M, N, gamma, st.invstd, dg2, db2, rw=rw)
    _, mag = bn_ref.bwd_finalize_terms(ws, M, gamma, st.invstd, r.gw, r.grows)
    for key, a, b in zip(("ca", "cb", "cc", "dgamma", "dbeta"), co + [dgamma, dbeta], list(fused) + [dg2, db2]):
        _within(a, b, 2 * U32 * mag[key], f"backward {key}")
