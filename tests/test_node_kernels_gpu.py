"""Every entry point of csrc/node.hip called on its own (node.node_gemm_desc / node.launch, ctypes
NodeBNDesc / NodeBNBwdDesc) and held to the float64 restatement tests/node_ref.py (pinned on the
CPU by tests/test_node_ref.py), at the smallest shapes where each path of the kernels exists:

  GEMM     M, N not multiples of the 32 x 32 tile; K with an empty lane half (K = 1, 15, 16), a
           partial one (17, 31, 47, 49), fewer K-chunks than waves, and exactly 8, 9 and 17 chunks
           (K = 256, 288, 544: one, two and three chunks for a wave, the v4 ring at every depth);
           k-contiguous / strided A and B, each 16-byte aligned (float4 / b128 loads) and as a view
           that breaks the alignment; A split along K (A2 / k1), B split along N (B2 / n1, also with
           a tile that straddles n1); every epilogue option alone and all together; zero sizes;
  v1 / v4  a K, k1, n1-aligned job runs on v4 when launched alone and on v1 when batched with a
           K = 45 job: both must agree bitwise, and both are compared with float64;
  colsum   1 .. 300 rows (one row lane, 16, 17, many), ragged N, accumulate on and off, M = 0;
  node BN  N around BN_COLS = 4 and row counts around BN_RL = 64, one to four sets, column-slice
           views with different row strides, relu_in on / off, training / eval (with the eval
           backward), dgamma / dbeta written and accumulated, two consecutive training calls;
  SyncBN   stats_out / stats_in and sums_out / sums_in with every set split over two unequal
           "ranks" in one process, merged on the host with node_ref.merge_stats.

Every output buffer is one row and several columns larger than the result and pre-filled with a
sentinel that must survive; operand padding is NaN, so a stray read that reaches a stored output
shows. Tolerance: tests/tol_check.py (3 x the float32 restatement's own error + 1e-5 / 2e-5 of the
largest float64 element). Decisions: the gate and the BN backward's Y > 0 are taken on inputs, which
the GPU and the references hold as the same fp32 numbers, so both sides decide alike; the ReLUs are
continuous in their argument (an argument within the tolerance of 0 moves the output by no more than
that), so no draw has to be rejected. A second run of every case is bitwise the first."""
import ctypes

import pytest
import torch

import node_ref as NR
from step_parity import report
from tol_check import F_FWD, F_GRAD, check

pytestmark = pytest.mark.gpu

SENT = -777.25
WORST = {}


@pytest.fixture(scope="module")
def hip(dev):
    from ured_hip import _lib, node
    return node, _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def out_buf(dev, M, N, old=None):
    """A result [M, N] inside a sentinel-filled [M + 1, N + 3] buffer -> (buffer, view)."""
    buf = torch.full((M + 1, N + 3), SENT, device=dev)
    if old is not None:
        buf[:M, :N] = old.to(dev)
    return buf, buf[:M, :N]


def intact(buf, M, N, what=""):
    assert bool((buf[M:] == SENT).all()) and bool((buf[:M, N:] == SENT).all()), f"{what}: wrote outside [0:{M}, 0:{N}]"


def place(mat, layout, aligned, dev):
    """mat [rows, K] (row = the operand's m or n index) on the device, NaN-padded ->
    (address, row stride, k stride, the buffer that owns the storage). layout "kc": k-contiguous
    rows; "st": stored transposed (unit row stride). aligned: 16-byte aligned rows; else a column
    slice starting at column 1 of a buffer with an odd row length. The address is the buffer's own
    (an empty view, K = 0 or an unused second source, has none to give)."""
    store = mat if layout == "kc" else mat.t()
    r, c = store.shape
    ld, o = ((c + 3) // 4 * 4 + 4, 0) if aligned else ((c + 2) | 1, 1)
    buf = torch.full((max(r, 1), ld), float("nan"), device=dev)
    buf[:r, o:o + c] = store.to(dev)
    addr = buf.data_ptr() + 4 * o
    assert (addr % 16 == 0 and ld % 4 == 0) == aligned
    return (addr, ld, 1, buf) if layout == "kc" else (addr, 1, ld, buf)


def side(mat, dev, extra=2, off=1):
    """An epilogue operand [M, N] as a column slice (row stride N + extra) -> (view, row stride)."""
    r, c = mat.shape
    buf = torch.full((r, c + extra), float("nan"), device=dev)
    buf[:, off:off + c] = mat.to(dev)
    return buf[:, off:off + c], c + extra


class Job:
    """One GEMM job: CPU fp32 data, its device operands in the asked layout, the descriptor and the
    restatement."""

    def __init__(self, dev, M, N, K, la="kc", lb="kc", aligned=True, k1=None, a_none=False, n1=None, lb2=None,
                 bias=False, rdiv=0, relu=False, gate=False, R_ncols=None, accumulate=False, seed=0):
        g = _gen(1000 * M + 100 * N + K + seed)
        self.M, self.N, self.K, self.k1, self.n1 = M, N, K, k1, n1
        A = torch.randn(M, K, generator=g)
        Bm = torch.randn(K, N, generator=g) / max(K, 1) ** 0.5
        ka = K if k1 is None else k1
        na = N if n1 is None else n1
        self.A = None if a_none else A[:, :ka]
        self.A2 = None if k1 is None else A[:, ka:]
        self.B, self.B2 = Bm[:, :na], (None if n1 is None else Bm[:, na:])
        self.bias = torch.randn(N, generator=g) if bias else None
        self.rdiv = rdiv
        self.rowbias = torch.randn((M + rdiv - 1) // rdiv, N, generator=g) if rdiv else None
        self.relu = relu
        self.gate = None
        if gate:                      # exact zeros, negatives and positives
            self.gate = torch.randn(M, N, generator=g)
            self.gate[torch.rand(M, N, generator=g) < 0.2] = 0.0
        self.R_ncols = R_ncols
        self.R = torch.randn(M, N, generator=g) if R_ncols is not None else None
        self.C_old = torch.randn(M, N, generator=g) if accumulate else None
        self.name = (f"M{M} N{N} K{K} A:{la} B:{lb} {'al' if aligned else 'un'}" + (f" k1={k1}" if k1 is not None else "") +
                     (" A=None" if a_none else "") + (f" n1={n1} B2:{lb2 or lb}" if n1 is not None else "") +
                     (" bias" if bias else "") + (f" rdiv={rdiv}" if rdiv else "") + (" relu" if relu else "") +
                     (" gate" if gate else "") + (f" R<{R_ncols}" if R_ncols is not None else "") +
                     (" acc" if accumulate else ""))
        # device operands
        z = (None, 0, 0, None)
        self.dA = z if self.A is None else place(self.A, la, aligned, dev)
        self.dA2 = z if self.A2 is None else place(self.A2, la, aligned, dev)
        self.dB = place(self.B.t(), lb, aligned, dev)
        self.dB2 = z if self.B2 is None else place(self.B2.t(), lb2 or lb, aligned, dev)
        self.dbias = None if self.bias is None else self.bias.to(dev)
        self.drb = (None, 0) if self.rowbias is None else side(self.rowbias, dev, 2, 0)
        self.dgate = (None, 0) if self.gate is None else side(self.gate, dev, 5, 3)
        self.dR = (None, 0) if self.R is None else side(self.R, dev, 1, 1)
        self.dev = dev

    def out(self):
        return out_buf(self.dev, self.M, self.N, self.C_old)

    def desc(self, node, C):
        (A, sam, sak), (A2, sam2, sak2), (B, sbn, sbk), (B2, sbn2, sbk2) = (t[:3] for t in (self.dA, self.dA2, self.dB, self.dB2))
        return node.node_gemm_desc(self.M, self.N, self.K, A, sam, sak, B, sbk, sbn, C, C.stride(0), A2=A2, sam2=sam2,
                                   sak2=sak2, k1=self.k1, B2=B2, sbk2=sbk2, sbn2=sbn2, n1=self.n1,
                                   accumulate=self.C_old is not None, bias=self.dbias, rowbias=self.drb[0],
                                   ldrb=self.drb[1], rdiv=max(self.rdiv, 1), relu_out=self.relu, gate=self.dgate[0],
                                   ldgate=self.dgate[1], R=self.dR[0], ldR=self.dR[1], R_ncols=self.R_ncols)

    def ref(self, dtype):
        return NR.gemm(self.A, self.B, A2=self.A2, B2=self.B2, bias=self.bias, rowbias=self.rowbias,
                       rdiv=max(self.rdiv, 1), relu=self.relu, gate=self.gate, R=self.R, R_ncols=self.R_ncols,
                       C_old=self.C_old, dtype=dtype)

    def v4_eligible(self):
        return (self.K > 0 and self.K % 32 == 0 and (self.k1 is None or self.k1 >= self.K or self.k1 % 32 == 0)
                and (self.n1 is None or self.n1 % 32 == 0))


def run(node, job, force_v1):
    """One launch of the job, alone (v4 when eligible) or batched with a K = 45 job (v1)."""
    buf, C = job.out()
    descs = [job.desc(node, C)]
    if force_v1:
        f = Job(job.dev, 5, 6, 45)
        fbuf, fC = f.out()
        descs.append(f.desc(node, fC))
    node.launch(*descs)
    intact(buf, job.M, job.N, job.name)
    if force_v1:
        intact(fbuf, 5, 6, "the K = 45 job")
    return C.clone()


def check_job(node, job):
    alone, again, v1 = run(node, job, False), run(node, job, False), run(node, job, True)
    assert torch.equal(alone, again), f"{job.name}: two runs differ"
    assert torch.equal(alone, v1), f"{job.name}: v1 and {'v4' if job.v4_eligible() else 'the single launch'} differ"
    check(WORST, "node GEMM", job.name, alone, job.ref(torch.float32), job.ref(torch.float64), F_FWD)


MS, NS = (1, 31, 33, 65), (1, 31, 33, 70)
KS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 256, 288, 544)
LAYOUTS = [(la, lb, al) for la in ("kc", "st") for lb in ("kc", "st") for al in (True, False)]


@pytest.mark.parametrize("K", KS)
def test_gemm_sizes_and_layouts(dev, hip, K):
    """Each K with ragged M and N (every value of M and of N appears across the K's, each with
    ragged values of the other two dimensions), in the four operand-layout combinations, aligned and
    not; the K-aligned ones on both kernels."""
    node, _ = hip
    i = KS.index(K)
    shapes = [(MS[i % 4], NS[(i + i // 4) % 4]), (MS[(i + 2) % 4], NS[(i + 1 + i // 4) % 4])]
    for q, (la, lb, al) in enumerate(LAYOUTS):
        M, N = shapes[q % 2]
        check_job(node, Job(dev, M, N, K, la, lb, al))


def test_gemm_dimension_coverage():
    """The shape table above pairs every M and every N with a ragged K, and every K with both."""
    seen_m, seen_n = set(), set()
    for i, K in enumerate(KS):
        for M, N in [(MS[i % 4], NS[(i + i // 4) % 4]), (MS[(i + 2) % 4], NS[(i + 1 + i // 4) % 4])]:
            if K % 32:
                seen_m.add(M), seen_n.add(N)
    assert seen_m == set(MS) and seen_n == set(NS)


@pytest.mark.parametrize("K,k1,a_none", [(96, 16, False), (96, 48, False), (96, 32, False), (96, 64, False),
                                         (45, 16, False), (50, 48, False), (64, 0, True), (64, 0, False),
                                         (64, 64, False), (45, 45, False)])
def test_gemm_split_a(dev, hip, K, k1, a_none):
    """cat([A, A2], 1) read in place: k1 = 16 / 48 (v1 only), 32 / 64 (v4 and v1), a partial last
    chunk inside A2, k1 = 0 with and without A, k1 = K with an A2 that is never read."""
    node, _ = hip
    for la, lb, al in LAYOUTS:
        check_job(node, Job(dev, 33, 70, K, la, lb, al, k1=k1, a_none=a_none))


@pytest.mark.parametrize("N,n1", [(70, 20), (70, 32), (70, 64), (33, 32), (70, 70)])
def test_gemm_split_b(dev, hip, N, n1):
    """Two column blocks B | B2: n1 = 20 (a tile straddles the split, each lane chooses its source:
    v1), 32 / 64 (v4 and v1), N - n1 = 50, 38, 6, 1 columns, n1 = N (B2 never read); B2 in the same
    and in the other layout than B."""
    node, _ = hip
    for K in (45, 64):
        for la, lb, al in LAYOUTS:
            for lb2 in ("kc", "st"):
                check_job(node, Job(dev, 33, N, K, la, lb, al, n1=n1, lb2=lb2))


@pytest.mark.parametrize("M,N,K1,K2", [(33, 45, 20, 50), (64, 70, 32, 38), (32, 5, 64, 6)])
def test_wgrad_desc_two_inputs(dev, hip, M, N, K1, K2):
    """wgrad_desc(g, x, C, x2=...): C [N, K1 + K2] = g^T cat([x, x2], 1), the weight gradient of the
    FFN's first convolution, x and x2 as column slices of one buffer; written and accumulated."""
    node, _ = hip
    gen = _gen(M + N + K1)
    g, big = torch.randn(M, N, generator=gen), torch.randn(M, K1 + K2 + 3, generator=gen)
    c0 = torch.randn(N, K1 + K2, generator=gen)
    gd, bigd = side(g, dev, 3, 2)[0], big.to(dev)
    x, x2 = bigd[:, :K1], bigd[:, K1 + 3:]
    xx = torch.cat([big[:, :K1], big[:, K1 + 3:]], 1)
    for acc in (False, True):
        outs = []
        for force in (False, False, True):
            buf, C = out_buf(dev, N, K1 + K2, c0 if acc else None)
            descs = [node.wgrad_desc(gd, x, C, accumulate=acc, x2=x2)]
            if force:
                f = Job(dev, 5, 6, 45)
                fbuf, fC = f.out()
                descs.append(f.desc(node, fC))
            node.launch(*descs)
            intact(buf, N, K1 + K2, "wgrad")
            outs.append(C.clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        ref = [NR.gemm(g.t(), xx[:, :K1], B2=xx[:, K1:], C_old=c0 if acc else None, dtype=dt)
               for dt in (torch.float32, torch.float64)]
        check(WORST, "node GEMM", f"wgrad x2 M{M} N{N} K{K1}+{K2} acc={acc}", outs[0], ref[0], ref[1], F_GRAD)


EPI = {"bias": dict(bias=True), "rowbias16": dict(rdiv=16), "rowbias5": dict(rdiv=5), "relu": dict(relu=True),
       "gate": dict(gate=True), "R_all": dict(R_ncols=70), "R_20": dict(R_ncols=20), "R_0": dict(R_ncols=0),
       "accumulate": dict(accumulate=True), "relu_gate": dict(relu=True, gate=True, bias=True),
       "all16": dict(bias=True, rdiv=16, relu=True, gate=True, R_ncols=20, accumulate=True),
       "all5": dict(bias=True, rdiv=5, relu=True, gate=True, R_ncols=70, accumulate=True)}


@pytest.mark.parametrize("opt", list(EPI))
def test_gemm_epilogue(dev, hip, opt):
    """Each epilogue option alone and all together at M = 33, N = 70 (a partial last row group, a
    row group that does not divide the tile, a gate with zeros and negatives read as a column slice,
    R on all / 20 / 0 columns, accumulation into a C with ldc > N), on v1 (K = 45) and on both
    kernels (K = 64), with a split A and B for the combined cases."""
    node, _ = hip
    for K in (45, 64):
        check_job(node, Job(dev, 33, 70, K, **EPI[opt]))
        check_job(node, Job(dev, 33, 70, K, "st", "st", False, **EPI[opt]))
    if opt.startswith("all"):
        check_job(node, Job(dev, 33, 70, 96, k1=32, n1=64, **EPI[opt]))
        check_job(node, Job(dev, 33, 70, 96, "kc", "st", False, k1=48, n1=20, lb2="kc", **EPI[opt]))


def _colsum_run(node, dev, g, c0, acc, extra=()):
    buf = torch.full((g.shape[1] + 3,), SENT, device=dev)
    if c0 is not None:
        buf[:g.shape[1]] = c0.to(dev)
    node.launch(node.colsum_desc(g, buf, accumulate=acc), *extra)
    assert bool((buf[g.shape[1]:] == SENT).all()), "colsum wrote past N"
    return buf[:g.shape[1]].clone()


@pytest.mark.parametrize("M", [1, 15, 16, 17, 300])
@pytest.mark.parametrize("N", [1, 33, 70])
def test_colsum(dev, hip, M, N):
    node, _ = hip
    gen = _gen(M * 100 + N)
    g, c0 = torch.randn(M, N, generator=gen), torch.randn(N, generator=gen)
    gd = side(g, dev, 4, 3)[0]
    for acc in (False, True):
        a, b = (_colsum_run(node, dev, gd, c0, acc) for _ in (0, 1))
        assert torch.equal(a, b)
        check(WORST, "node colsum", f"M{M} N{N} acc={acc}", a, NR.colsum(g, c0, acc, torch.float32),
              NR.colsum(g, c0, acc), F_GRAD)


def test_zero_sizes(dev, hip):
    """K = 0: the GEMM writes its epilogue only. M = 0 column sum: zeros, or C unchanged when it
    accumulates (the job used to be skipped, leaving C unwritten), alone and beside another job,
    from a zero-row slice and from an empty tensor (null address). An M = 0 or N = 0 GEMM writes
    nothing."""
    node, _ = hip
    check_job(node, Job(dev, 33, 70, 0, bias=True, rdiv=5, relu=True, R_ncols=20, accumulate=True))
    check_job(node, Job(dev, 5, 3, 0))
    c0 = torch.randn(70, generator=_gen(5))
    other = Job(dev, 33, 31, 47)
    obuf, oC = other.out()                # held: the descriptor carries its address only
    for g in (torch.randn(4, 75, device=dev)[:0, 2:72], torch.empty(0, 70, device=dev)):
        for extra in ((), (other.desc(node, oC),)):
            assert torch.equal(_colsum_run(node, dev, g, None, False, extra), torch.zeros(70, device=dev))
            assert torch.equal(_colsum_run(node, dev, g, c0, True, extra), c0.to(dev))
    intact(obuf, 33, 31, other.name)
    check(WORST, "node GEMM", "beside an M = 0 colsum " + other.name, oC, other.ref(torch.float32), other.ref(torch.float64), F_FWD)
    for M, N in ((0, 7), (7, 0)):
        buf = torch.full((8, 10), SENT, device=dev)
        x, W = torch.randn(max(M, 1), 16, device=dev), torch.randn(max(N, 1), 16, device=dev)
        node.launch(node.linear_desc(x[:M], W[:N], buf[:M, :N]))
        assert bool((buf == SENT).all())


def test_batched_mixed_jobs_equal_single_launches(dev, hip):
    """Six jobs of mixed kinds in one launch (a K-aligned GEMM with every epilogue option, a K = 45
    GEMM that puts the launch on v1, an M = 0 GEMM in the middle, a split-B GEMM, a one-row
    strided GEMM, a column sum) equal the single launches (v4 where eligible) bitwise."""
    node, _ = hip
    jobs = [Job(dev, 33, 70, 64, **EPI["all16"]), Job(dev, 65, 31, 45, "st", "kc", False, bias=True),
            Job(dev, 31, 33, 288, "kc", "st", True, n1=32, lb2="kc"), Job(dev, 1, 70, 32, "st", "st", False, relu=True)]
    g = torch.randn(17, 33, generator=_gen(2))
    gd = side(g, dev, 4, 1)[0]
    x0, W0 = torch.randn(4, 32, device=dev), torch.randn(9, 32, device=dev)

    def launch_all(batched):
        outs = [j.out() for j in jobs]
        cs = torch.full((36,), SENT, device=dev)
        e = torch.full((3, 12), SENT, device=dev)
        descs = [j.desc(node, o[1]) for j, o in zip(jobs, outs)]
        descs = descs[:2] + [node.linear_desc(x0[:0], W0, e[:0, :9])] + descs[2:] + [node.colsum_desc(gd, cs)]
        assert len(descs) == node.MAX_JOBS
        if batched:
            node.launch(*descs)
        else:
            for d in descs:
                node.launch(d)
        for j, (buf, _) in zip(jobs, outs):
            intact(buf, j.M, j.N, j.name)
        assert bool((e == SENT).all()) and bool((cs[33:] == SENT).all())
        return [o[1].clone() for o in outs] + [cs[:33].clone()]

    one, two, single = launch_all(True), launch_all(True), launch_all(False)
    for a, b, c in zip(one, two, single):
        assert torch.equal(a, b) and torch.equal(a, c)
    for j, o in zip(jobs, one):
        check(WORST, "node GEMM", "batched " + j.name, o, j.ref(torch.float32), j.ref(torch.float64), F_FWD)
    check(WORST, "node colsum", "batched", one[-1], NR.colsum(g, dtype=torch.float32), NR.colsum(g), F_GRAD)


# ---- node BatchNorm ----------------------------------------------------------------------------

MOM, EPS = 0.3, 1e-3


def _off_arr(node, off):
    return (ctypes.c_int * (node.MAX_SETS + 1))(*(list(off) + [off[-1]] * (node.MAX_SETS + 1 - len(off))))


def _flat(dev, n, vals=None):
    """[n] inside a sentinel-tailed [n + 3] buffer."""
    buf = torch.full((n + 3,), SENT, device=dev)
    if vals is not None:
        buf[:n] = vals.reshape(-1).to(dev)
    return buf


def _tail_ok(buf, n, what):
    assert bool((buf[n:] == SENT).all()), f"{what}: wrote past its {n} elements"


class BNState:
    """Device-side module state of one "rank": gamma, beta, running statistics, num_batches_tracked."""

    def __init__(self, dev, gamma, beta, rm, rv, nbt):
        N = gamma.numel()
        self.N, self.dev = N, dev
        self.gamma, self.beta = gamma.to(dev), beta.to(dev)
        self.rm, self.rv = _flat(dev, N, rm), _flat(dev, N, rv)
        self.nbt = torch.tensor([nbt, -5], dtype=torch.int64, device=dev)

    def check_tails(self):
        _tail_ok(self.rm, self.N, "running_mean"), _tail_ok(self.rv, self.N, "running_var")
        assert int(self.nbt[1]) == -5


def bn_fwd(hip, st, Yv, off, training, relu_in, stats_out=None, stats_in=None):
    """ured_node_bn_fwd on the view Yv -> (act view [R, N] of a sentinel buffer, mean, invstd [S, N])."""
    node, lib = hip
    dev, N, S, R = st.dev, st.N, len(off) - 1, Yv.shape[0]
    abuf = torch.full((R + 1, N + 3), SENT, device=dev)
    mean, invstd = _flat(dev, S * N), _flat(dev, S * N)
    d = node.NodeBNDesc()
    d.N, d.nsets, d.off = N, S, _off_arr(node, off)
    d.Y, d.ldy, d.relu_in, d.training = Yv.data_ptr(), Yv.stride(0), int(relu_in), int(training)
    d.gamma, d.beta = st.gamma.data_ptr(), st.beta.data_ptr()
    d.running_mean, d.running_var = st.rm.data_ptr(), st.rv.data_ptr()
    d.num_batches_tracked = st.nbt.data_ptr() if training else None
    d.momentum, d.eps = MOM, EPS
    d.mean, d.invstd = mean.data_ptr(), invstd.data_ptr()
    d.act, d.ld_act = abuf.data_ptr(), abuf.stride(0)
    d.stats_out = None if stats_out is None else stats_out.data_ptr()
    d.stats_in = None if stats_in is None else stats_in.data_ptr()
    lib.call("ured_node_bn_fwd", ctypes.byref(d), lib.current_stream())
    intact(abuf, R, N, "BN act")
    _tail_ok(mean, S * N, "mean"), _tail_ok(invstd, S * N, "invstd")
    st.check_tails()
    return abuf, mean, invstd


def bn_bwd(hip, st, Gv, Yv, off, mean, invstd, training, relu_in, dg0=None, db0=None, sums_out=None, sums_in=None):
    """ured_node_bn_bwd -> (dY buffer, dgamma, dbeta buffers); dg0 / db0: accumulate into them."""
    node, lib = hip
    dev, N, S, R = st.dev, st.N, len(off) - 1, Yv.shape[0]
    dbuf = torch.full((R + 1, N + 4), SENT, device=dev)
    dgamma, dbeta = _flat(dev, N, dg0), _flat(dev, N, db0)
    d = node.NodeBNBwdDesc()
    d.N, d.nsets, d.off = N, S, _off_arr(node, off)
    d.G, d.ldg = Gv.data_ptr(), Gv.stride(0)
    d.Y, d.ldy, d.relu_in, d.training = Yv.data_ptr(), Yv.stride(0), int(relu_in), int(training)
    d.gamma, d.mean, d.invstd = st.gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    d.dY, d.lddy = dbuf.data_ptr(), dbuf.stride(0)
    d.dgamma, d.dbeta, d.accumulate = dgamma.data_ptr(), dbeta.data_ptr(), int(dg0 is not None)
    d.sums_out = None if sums_out is None else sums_out.data_ptr()
    d.sums_in = None if sums_in is None else sums_in.data_ptr()
    lib.call("ured_node_bn_bwd", ctypes.byref(d), lib.current_stream())
    intact(dbuf, R, N, "BN dY")
    _tail_ok(dgamma, N, "dgamma"), _tail_ok(dbeta, N, "dbeta")
    return dbuf, dgamma, dbeta


def _bn_data(N, sizes, seed):
    g = _gen(seed)
    R = sum(sizes)
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    d = {"off": off, "Y": [torch.randn(R, N, generator=g) + 0.3 for _ in (0, 1)],
         "G": torch.randn(R, N, generator=g), "gamma": torch.randn(N, generator=g) + 0.2,
         "beta": torch.randn(N, generator=g), "rm": 0.1 * torch.randn(N, generator=g),
         "rv": torch.rand(N, generator=g) + 0.5, "dg0": torch.randn(N, generator=g), "db0": torch.randn(N, generator=g)}
    if N > 1:
        d["gamma"][0], d["gamma"][1] = -d["gamma"][0].abs() - 0.1, d["gamma"][1].abs() + 0.1   # both signs
    return d


BN_CASES = [(1, (2,)), (3, (63, 64)), (4, (65, 130, 2)), (5, (64, 2, 63, 65)), (70, (130, 65)), (5, (130,)), (4, (2, 2, 2, 2))]


@pytest.mark.parametrize("N,sizes", BN_CASES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu_in", [True, False])
def test_node_bn(dev, hip, N, sizes, training, relu_in):
    D = _bn_data(N, sizes, 17 * N + len(sizes) + 2 * training + relu_in)
    off, R, S = D["off"], sum(sizes), len(sizes)

    def gpu():
        st = BNState(dev, D["gamma"], D["beta"], D["rm"], D["rv"], 3)
        res = {}
        for call in (0, 1):           # two consecutive calls: the running statistics compound
            Yv = side(D["Y"][call], dev, 5, 2)[0]
            abuf, mean, invstd = bn_fwd(hip, st, Yv, off, training, relu_in)
            res[f"act{call}"], res[f"mean{call}"], res[f"invstd{call}"] = abuf[:R, :N].clone(), mean[:S * N], invstd[:S * N]
            res[f"rm{call}"], res[f"rv{call}"], res[f"nbt{call}"] = st.rm[:N].clone(), st.rv[:N].clone(), int(st.nbt[0])
        Gv = side(D["G"], dev, 2, 1)[0]
        dbuf, dgamma, dbeta = bn_bwd(hip, st, Gv, Yv, off, mean, invstd, training, relu_in)
        _, dg_acc, db_acc = bn_bwd(hip, st, Gv, Yv, off, mean, invstd, training, relu_in, D["dg0"], D["db0"])
        res.update(dY=dbuf[:R, :N].clone(), dgamma=dgamma[:N], dbeta=dbeta[:N], dg_acc=dg_acc[:N], db_acc=db_acc[:N])
        return res

    def ref(dt):
        res, rm, rv, nbt = {}, D["rm"], D["rv"], 3
        for call in (0, 1):
            r = NR.bn_sets(D["Y"][call], off, D["gamma"], D["beta"], rm, rv, MOM, EPS, training, relu_in, nbt, dtype=dt)
            rm, rv, nbt = r["running_mean"], r["running_var"], r["num_batches_tracked"]
            res[f"act{call}"], res[f"mean{call}"], res[f"invstd{call}"] = r["act"], r["mean"].reshape(-1), r["invstd"].reshape(-1)
            res[f"rm{call}"], res[f"rv{call}"], res[f"nbt{call}"] = rm, rv, nbt
        dY, dg, db = NR.bn_sets_bwd(D["G"], D["Y"][1], off, D["gamma"], r["mean"], r["invstd"], training, relu_in, dtype=dt)
        res.update(dY=dY, dgamma=dg, dbeta=db, dg_acc=dg + D["dg0"].to(dt), db_acc=db + D["db0"].to(dt))
        return res

    a, b, r32, r64 = gpu(), gpu(), ref(torch.float32), ref(torch.float64)
    name = f"N{N} sets{sizes} train={int(training)} relu={int(relu_in)}"
    for k in a:
        if k.startswith("nbt"):
            assert a[k] == b[k] == r64[k] == 3 + (int(k[3:]) + 1) * S * training, (k, a[k], r64[k])
            continue
        assert torch.equal(a[k], b[k]), f"{name} {k}: two runs differ"
        grad = k in ("dY", "dgamma", "dbeta", "dg_acc", "db_acc")
        check(WORST, "node BN bwd" if grad else "node BN fwd", f"{name} {k}", a[k], r32[k], r64[k], F_GRAD if grad else F_FWD)
    if not training:                   # eval leaves the module alone
        assert torch.equal(a["rm1"].cpu(), D["rm"]) and torch.equal(a["rv1"].cpu(), D["rv"])


@pytest.mark.parametrize("N,splits", [(5, ((5, 60), (100, 30))), (4, ((1, 1),)), (3, ((64, 1), (2, 63), (33, 32), (1, 129)))])
@pytest.mark.parametrize("relu_in", [True, False])
def test_node_syncbn_modes_two_ranks(dev, hip, N, splits, relu_in):
    """Every set split over two unequal "ranks": stats_out per rank, merged on the host
    (node_ref.merge_stats), stats_in per rank -> each rank's acts are the full set's rows, mean /
    invstd / running statistics the full set's; sums_out per rank, summed, sums_in -> dY the full
    set's rows, the ranks' dgamma / dbeta add up to the full set's."""
    sizes = [a + b for a, b in splits]
    D = _bn_data(N, sizes, 7 * N + len(sizes) + relu_in)
    off, S = D["off"], len(sizes)
    Y, G = D["Y"][0], D["G"]
    rows = [[], []]                       # each rank's row indices, set by set
    roff = [[0], [0]]
    for s, (na, nb) in enumerate(splits):
        rows[0] += list(range(off[s], off[s] + na))
        rows[1] += list(range(off[s] + na, off[s + 1]))
        roff[0].append(roff[0][-1] + na)
        roff[1].append(roff[1][-1] + nb)

    def gpu():
        sts = [BNState(dev, D["gamma"], D["beta"], D["rm"], D["rv"], 3) for _ in (0, 1)]
        Yv = [side(Y[rows[r]], dev, 5, 2)[0] for r in (0, 1)]
        Gv = [side(G[rows[r]], dev, 2, 1)[0] for r in (0, 1)]
        local = [torch.full((S * 3 * N + 3,), float(SENT), dtype=torch.float64, device=dev) for _ in (0, 1)]
        for r in (0, 1):
            before = (sts[r].rm.clone(), sts[r].rv.clone())
            node, lib = hip
            # stats_out writes nothing else: act / mean / invstd may be null
            d = node.NodeBNDesc()
            d.N, d.nsets, d.off = N, S, _off_arr(node, roff[r])
            d.Y, d.ldy, d.relu_in, d.training = Yv[r].data_ptr(), Yv[r].stride(0), int(relu_in), 1
            d.gamma, d.beta = sts[r].gamma.data_ptr(), sts[r].beta.data_ptr()
            d.running_mean, d.running_var, d.num_batches_tracked = sts[r].rm.data_ptr(), sts[r].rv.data_ptr(), sts[r].nbt.data_ptr()
            d.momentum, d.eps, d.stats_out = MOM, EPS, local[r].data_ptr()
            lib.call("ured_node_bn_fwd", ctypes.byref(d), lib.current_stream())
            assert torch.equal(sts[r].rm, before[0]) and torch.equal(sts[r].rv, before[1]) and int(sts[r].nbt[0]) == 3
            assert bool((local[r][S * 3 * N:] == SENT).all())
        st = [loc[:S * 3 * N].view(S, 3, N).cpu() for loc in local]
        merged = torch.stack([NR.merge_stats(st[0][s], st[1][s]) for s in range(S)])
        res = {"stats0": st[0], "stats1": st[1], "merged": merged}
        glob = merged.to(dev)
        fw = [bn_fwd(hip, sts[r], Yv[r], roff[r], True, relu_in, stats_in=glob) for r in (0, 1)]
        sums = [torch.full((S * 3 * N + 3,), float(SENT), dtype=torch.float64, device=dev) for _ in (0, 1)]
        for r in (0, 1):
            node, lib = hip
            d = node.NodeBNBwdDesc()
            d.N, d.nsets, d.off = N, S, _off_arr(node, roff[r])
            d.G, d.ldg, d.Y, d.ldy = Gv[r].data_ptr(), Gv[r].stride(0), Yv[r].data_ptr(), Yv[r].stride(0)
            d.relu_in, d.training = int(relu_in), 1
            d.gamma, d.mean, d.invstd = sts[r].gamma.data_ptr(), fw[r][1].data_ptr(), fw[r][2].data_ptr()
            d.sums_out = sums[r].data_ptr()
            lib.call("ured_node_bn_bwd", ctypes.byref(d), lib.current_stream())
            assert bool((sums[r][S * 3 * N:] == SENT).all())
        tot = (sums[0][:S * 3 * N] + sums[1][:S * 3 * N]).contiguous()
        bw = [bn_bwd(hip, sts[r], Gv[r], Yv[r], roff[r], fw[r][1], fw[r][2], True, relu_in, sums_in=tot) for r in (0, 1)]
        act, dY = torch.empty(off[-1], N), torch.empty(off[-1], N)
        for r in (0, 1):
            act[rows[r]] = fw[r][0][:len(rows[r]), :N].cpu()
            dY[rows[r]] = bw[r][0][:len(rows[r]), :N].cpu()
            res[f"mean{r}"], res[f"invstd{r}"] = fw[r][1][:S * N].clone(), fw[r][2][:S * N].clone()
            res[f"rm{r}"], res[f"rv{r}"] = sts[r].rm[:N].clone(), sts[r].rv[:N].clone()
            assert int(sts[r].nbt[0]) == 3 + S
        res.update(act=act, dY=dY, sums=tot.view(S, 3, N).cpu(), dgamma=bw[0][1][:N] + bw[1][1][:N], dbeta=bw[0][2][:N] + bw[1][2][:N])
        return res

    def ref(dt):
        r = NR.bn_sets(Y, off, D["gamma"], D["beta"], D["rm"], D["rv"], MOM, EPS, True, relu_in, 3, dtype=dt)
        dY, dg, db = NR.bn_sets_bwd(G, Y, off, D["gamma"], r["mean"], r["invstd"], True, relu_in, dtype=dt)
        res = {"act": r["act"], "dY": dY, "dgamma": dg, "dbeta": db}
        for q in (0, 1):
            res[f"mean{q}"], res[f"invstd{q}"] = r["mean"].reshape(-1), r["invstd"].reshape(-1)
            res[f"rm{q}"], res[f"rv{q}"] = r["running_mean"], r["running_var"]
            res[f"stats{q}"] = torch.stack([NR.bn_rank_stats(Y[rows[q]][roff[q][s]:roff[q][s + 1]], relu_in, dt) for s in range(S)])
        res["merged"] = torch.stack([NR.bn_rank_stats(Y[off[s]:off[s + 1]], relu_in, dt) for s in range(S)])
        res["sums"] = torch.stack([NR.bn_rank_sums(G[off[s]:off[s + 1]], Y[off[s]:off[s + 1]], r["mean"][s], r["invstd"][s],
                                                   relu_in, dt) for s in range(S)])
        return res

    a, b, r32, r64 = gpu(), gpu(), ref(torch.float32), ref(torch.float64)
    name = f"N{N} splits{splits} relu={int(relu_in)}"
    for k in r64:
        assert torch.equal(a[k], b[k]), f"{name} {k}: two runs differ"
        grad = k in ("dY", "dgamma", "dbeta", "sums")
        check(WORST, "node SyncBN", f"{name} {k}", a[k], r32[k], r64[k], F_GRAD if grad else F_FWD)
    assert torch.equal(a["rm0"], a["rm1"]) and torch.equal(a["rv0"], a["rv1"]) and torch.equal(a["mean0"], a["mean1"])
    assert torch.equal(a["stats0"][:, 0], torch.tensor([[float(x[0])] * N for x in splits], dtype=torch.float64))


def test_report_worst_ratios():
    """Not a check: the worst err / tolerance measured above, per kernel family."""
    for fam, (ratio, what) in sorted(WORST.items()):
        report(f"node kernel parity, {fam}: worst err / tolerance {ratio:.3f} ({what})")
