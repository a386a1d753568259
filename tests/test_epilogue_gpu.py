"""The MFMA kernels' EPI_BNBWD and EPI_FWD epilogues of ured_gemm (csrc/mlp.hip epilogue() /
bnbwd_full(), reached from gemm2_kernel and gemm_kernel) against float64, one launch per case.
K >= 8 (or K = 0) throughout, so the K <= 4 streaming kernels of tests/test_edge_gpu.py are not taken.

Every case id names the kernel the dispatcher picks for it (launch(): vec_ok / v2_ok / buf_ok,
restated in _route() below and asserted, so an id cannot drift from the code path):
  gemm2_tn2    gemm2_kernel, 128 x 128 tile (TN = 2), buffer stores (BUFST): the only kernel that
               can take bnbwd_full
  gemm2_tn1    gemm2_kernel, 128 x 64 tile (TN = 1), N <= 64
  gemm_vec     gemm_kernel<..., VEC = true>  (float4 operand loads, plain stores)
  gemm_scalar  gemm_kernel<..., VEC = false>

EPI_BNBWD branches, M = 300 = row tiles 0, 1 (full) + tile 2 (44 valid rows):
  plain     gemm2: bnbwd_full<POOL = false> on full tiles, the general loop (fast form) on the
            partial row tile and the partial column tile; gemm_kernel: general loop (fast) only
  gadd      the general loop's slow (per-element) form on every tile
  pool128 / pool256   pooled gradient of 128-row-aligned groups: bnbwd_full<POOL = true> on full
            tiles, pool_blk in the general loop (fast form) elsewhere
  pool100 / pool150   groups that do not align with the row block: per-element pool_idx reads in
            the general loop's slow form
each under the three activation orders ACT_ENC / ACT_RES / ACT_BN. ACT_RES cases also give C and
Yp a row pitch of N + 4 (ldc, ldy > N). Tolerances are those of test_dgrad_small_bnbwd: G within
1e-5 * (1 + max |ref|), each block's two partials rtol = atol = 1e-4. BN scales are +-2^k and
shifts quarter integers, so y*scale+shift is exact in float64 and has the sign of the kernel's
fp32 fma: the ReLU masks agree exactly, under negative scales too.

EPI_FWD: Y within 1e-5 of max |ref| (as test_gemm_prologue_stats), block partials with the
test_fwd_small_stats tolerances (mean rtol = atol = 1e-5, M2 rtol = atol = 1e-4), and the pool
records exactly: the max / min of the stored fp32 Y rows of the block, lowest row on ties."""
import pytest
import torch

import bn_ref

pytestmark = pytest.mark.gpu

SENT = -777.25      # sentinel for memory the kernels must not write


@pytest.fixture(scope="module")
def K(dev):
    from ured_hip import kernels
    return kernels


def _route(N, Kd, lda, ldb, b_kmajor, pro_a=0, k1=None, lda2=0):
    """launch() of csrc/mlp.hip for row-major A, 16-byte aligned operands, K outside 1..4."""
    k1 = Kd if k1 is None else k1
    vec = (lda % 4 == 0 and Kd % 4 == 0 and k1 % 4 == 0 and (k1 == Kd or lda2 % 4 == 0) and ldb % 4 == 0 and
           (N % 4 == 0 if b_kmajor else Kd % 4 == 0))
    v2 = not (pro_a and k1 % 16 != 0) and Kd >= 4 and not (b_kmajor and N < 4)
    buf = k1 >= Kd or k1 % 32 == 0
    if vec and v2 and buf:
        return "gemm2_tn1" if N <= 64 else "gemm2_tn2"
    return "gemm_vec" if vec else "gemm_scalar"


def _close_max(got, ref, rel, name):
    err = (got.double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= rel * scale, f"{name}: max err {err:.3e} > {rel:.0e} * {scale:.3e}"


# ------------------------------------------------------------------ EPI_BNBWD

# id, M, N, K, ldb, kernel
BNBWD_SHAPES = [
    ("300x192x32-gemm2_tn2-full_tiles+partial_row_and_col_tile", 300, 192, 32, 192, "gemm2_tn2"),
    ("300x64x32-gemm2_tn1-full_col_tile", 300, 64, 32, 64, "gemm2_tn1"),
    ("300x40x32-gemm2_tn1-partial_col_tile", 300, 40, 32, 40, "gemm2_tn1"),
    ("300x70x8-gemm_scalar-N%4", 300, 70, 8, 70, "gemm_scalar"),
    ("300x132x8-gemm_scalar-ldb133", 300, 132, 8, 133, "gemm_scalar"),
    ("129x128x0-gemm_vec-K0", 129, 128, 0, 128, "gemm_vec"),
]
BNBWD_VARIANTS = ["plain", "gadd", "pool128", "pool256", "pool100", "pool150"]
MODES = [(bn_ref.ACT_ENC, "enc"), (bn_ref.ACT_RES, "res"), (bn_ref.ACT_BN, "bn")]


def _pool_winners(M, N, pgr):
    """pool_idx [G][N] chosen by hand: per group the first and the last row, rows 127 / 128 and
    M - 1 where they fall in the group, and rows of every (wave half wm, lane half) of a 128-row
    tile: tile row tr = row % 128 has wm = tr // 64 and sits in lanes >= 32 iff tr % 8 >= 4
    (+0: wm 0 lanes < 32, +5 / +37: wm 0 lanes >= 32, +64 / +97: wm 1 lanes < 32, +70 / +100:
    wm 1 lanes >= 32, for a group that starts on a tile)."""
    G = (M + pgr - 1) // pgr
    idx = torch.empty(G, N, dtype=torch.int32)
    for g in range(G):
        lo, hi = g * pgr, min(M, (g + 1) * pgr)
        cand = [lo, hi - 1] + [r for r in (lo + 5, lo + 37, lo + 64, lo + 70, lo + 97, lo + 100, 127, 128, M - 1)
                               if lo < r < hi - 1]
        for n in range(N):
            idx[g, n] = cand[(n + g) % len(cand)]
    return idx


@pytest.mark.parametrize("mode,mname", MODES, ids=[m[1] for m in MODES])
@pytest.mark.parametrize("variant", BNBWD_VARIANTS)
@pytest.mark.parametrize("cid,M,N,Kd,ldb,kernel", BNBWD_SHAPES, ids=[s[0] for s in BNBWD_SHAPES])
def test_bnbwd_epilogue(K, dev, cid, M, N, Kd, ldb, kernel, variant, mode, mname):
    lda = max(Kd, 4)
    assert _route(N, Kd, lda, ldb, True) == kernel
    g = torch.Generator().manual_seed(1000 * M + 10 * N + Kd + mode)
    pad = 4 if mode == bn_ref.ACT_RES else 0          # ldc, ldy > N
    dY = torch.randn(M, lda, generator=g)
    W = torch.randn(max(Kd, 1), ldb, generator=g) * max(Kd, 1) ** -0.5      # k-major B: W[k][n]
    Yp = torch.randn(M, N, generator=g)
    mean = torch.randn(N, generator=g) * 0.1
    invstd = torch.rand(N, generator=g) + 0.5
    scale = torch.randint(-1, 2, (N,), generator=g).float().exp2() * (torch.randint(0, 2, (N,), generator=g).float() * 2 - 1)
    shift = torch.randint(-2, 3, (N,), generator=g).float() * 0.25
    assert (scale < 0).any() and (scale > 0).any()
    ga = torch.randn(M, N, generator=g) if variant == "gadd" else None
    pidx = pgrad = None
    pgr = 0
    if variant.startswith("pool"):
        pgr = int(variant[4:])
        pidx = _pool_winners(M, N, pgr)
        pgrad = torch.randn(pidx.shape[0], N, generator=g)

    Cbuf = torch.full((M + 2, N + pad), SENT, device=dev)
    Ybuf = torch.zeros(M, N + pad, device=dev)
    Ybuf[:, :N] = Yp.to(dev)
    ws = torch.full((2, N, K.nblocks(M)), SENT, device=dev)      # [2][N][blocks] (include/ured_hip.h)
    bn = K.BNState(mean.to(dev), invstd.to(dev), scale.to(dev), shift.to(dev))
    K.gemm(M, N, Kd, dY.to(dev), lda, W.to(dev), ldb, Cbuf, N + pad, b_kmajor=True, epi=K.EPI_BNBWD, Yp=Ybuf,
           ldy=N + pad, bn=bn, bwd_res=mode, bwd_ws=ws, gadd=None if ga is None else ga.to(dev),
           ldg=N if ga is not None else 0, pool_idx=None if pidx is None else pidx.to(dev),
           pool_grad=None if pgrad is None else pgrad.to(dev), pool_group_rows=pgr)

    dh = dY[:, :Kd].double() @ W[:Kd, :N].double()
    if pidx is not None:
        dh.scatter_add_(0, pidx.long(), pgrad.double())          # the pooled gradient lands on the winning row
    if ga is not None:
        dh = dh + ga.double()
    gr, _, xh = bn_ref.act_terms(dh, Yp, mode, mean, invstd, scale, shift)
    C = Cbuf.cpu()
    assert (C[:M, :N].double() - gr).abs().max().item() <= 1e-5 * (1 + gr.abs().max().item())
    assert (C[M:] == SENT).all(), "rows >= M of C written"
    assert (C[:M, N:] == SENT).all(), "columns >= N of C written"
    ref = bn_ref.block_bwd_partials(gr, xh)
    got = ws.cpu().double()
    for blk in range(K.nblocks(M)):
        assert torch.allclose(got[0, :, blk], ref[0, :, blk], rtol=1e-4, atol=1e-4), f"sum g, block {blk}"
        assert torch.allclose(got[1, :, blk], ref[1, :, blk], rtol=1e-4, atol=1e-4), f"sum g*xhat, block {blk}"


# ------------------------------------------------------------------ EPI_FWD

FWD_SHAPES = [(300, 192, 32), (300, 40, 32), (257, 70, 36)]
# kernel by (shape, prologue?): a prologue needs k1 % 16 == 0 for gemm2 (v2_ok)
FWD_KERNEL = {(300, 192, 32, False): "gemm2_tn2", (300, 192, 32, True): "gemm2_tn2",
              (300, 40, 32, False): "gemm2_tn1", (300, 40, 32, True): "gemm2_tn1",
              (257, 70, 36, False): "gemm2_tn2", (257, 70, 36, True): "gemm_vec"}
# (pro_a, stat_relu): the statistics are of relu(Y) in a Conv -> ReLU -> BN chain
FWD_PRO = [(0, False, "pro_none"), (0, True, "pro_none_statrelu"), (1, False, "pro_enc"), (2, True, "pro_res")]
FWD_RB = ["bias", "rb128_rb_blk_shortcut", "rb120_per_element", "gidx_ragged_per_element"]


def _pro(X, pro, s, t):
    X = X.double()
    if pro == 1:
        return torch.relu(X * s.double() + t.double())
    if pro == 2:
        return torch.relu(X) * s.double() + t.double()
    return X


def _rowbias(M, N, rb, g):
    """-> (rowbias [G][N+4] or None, kwargs of K.gemm, group of every row)."""
    if rb == "bias":
        return None, {}, None
    if rb.startswith("gidx"):
        sizes = [70, 0, 129, 1, M - 200]                     # ragged, one empty group
        grp = torch.repeat_interleave(torch.arange(5), torch.tensor(sizes))
    else:
        gr = int(rb[2:5])
        grp = torch.arange(M) // gr
    R = torch.randn(int(grp.max()) + 1, N + 4, generator=g)
    if rb.startswith("gidx"):
        return R, {"gidx": grp.int()}, grp
    return R, {"group_rows": gr}, grp


def _check_fwd(K, Y, ws, ref, M, N, stat_relu, name):
    _close_max(Y, ref, 1e-5, name)
    p = ref.clamp_min(0) if stat_relu else ref
    want = bn_ref.block_partials(p)
    got = ws.cpu().double()
    for blk in range(K.nblocks(M)):
        assert torch.allclose(got[0, :, blk], want[0, :, blk], rtol=1e-5, atol=1e-5), f"{name}: mean, block {blk}"
        assert torch.allclose(got[1, :, blk], want[1, :, blk], rtol=1e-4, atol=1e-4), f"{name}: M2, block {blk}"


@pytest.mark.parametrize("rb", FWD_RB)
@pytest.mark.parametrize("pro,stat_relu,pname", FWD_PRO, ids=[p[2] for p in FWD_PRO])
@pytest.mark.parametrize("M,N,Kd", FWD_SHAPES, ids=lambda v: str(v))
def test_fwd_epilogue(K, dev, M, N, Kd, pro, stat_relu, pname, rb):
    kernel = FWD_KERNEL[(M, N, Kd, pro != 0)]
    assert _route(N, Kd, Kd, Kd, False, pro_a=pro) == kernel
    g = torch.Generator().manual_seed(M + 7 * N + Kd + pro)
    X = torch.randn(M, Kd, generator=g)
    W = torch.randn(N, Kd, generator=g) * Kd ** -0.5
    b = torch.randn(N, generator=g)
    s, t = torch.rand(Kd, generator=g) + 0.5, torch.randn(Kd, generator=g)
    R, kw, grp = _rowbias(M, N, rb, g)
    if R is not None:
        kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
        kw.update(rowbias=R.to(dev), ldr=N + 4)
    if pro:
        kw.update(pro_a=pro, pro_s=s.to(dev), pro_t=t.to(dev))
    Ybuf = torch.full((M + 2, N + 4), SENT, device=dev)
    ws = torch.full((2, N, K.nblocks(M)), SENT, device=dev)
    K.gemm(M, N, Kd, X.to(dev), Kd, W.to(dev), Kd, Ybuf, N + 4, epi=K.EPI_FWD, bias=b.to(dev), stat_ws=ws,
           stat_relu=stat_relu, **kw)
    ref = _pro(X, pro, s, t) @ W.double().t() + b.double()
    if R is not None:
        ref = ref + R[grp, :N].double()
    Yc = Ybuf.cpu()
    assert (Yc[M:] == SENT).all() and (Yc[:M, N:] == SENT).all(), "C written outside [M][N]"
    _check_fwd(K, Yc[:M, :N], ws, ref, M, N, stat_relu, f"{kernel} {pname} {rb}")


# A2 / k1 concatenation: A'[m][k] = k < k1 ? pro(A[m][k]) : A2[m][k - k1]; the prologue's
# channel vectors have k1 entries. Kernel by form: k1 % 32 == 0 keeps gemm2 (buf_ok); k1 % 4 == 0
# only is the vector gemm_kernel; k1 % 4 != 0 the scalar one.
CONCAT = [("k1_32_of_64-gemm2_tn2", 64, 32, "gemm2_tn2"), ("k1_20_of_36-gemm_vec", 36, 20, "gemm_vec"),
          ("k1_18_of_36-gemm_scalar", 36, 18, "gemm_scalar")]


@pytest.mark.parametrize("pro,stat_relu,pname", FWD_PRO[1:], ids=[p[2] for p in FWD_PRO[1:]])
@pytest.mark.parametrize("M,N", [(300, 192), (257, 70)], ids=lambda v: str(v))
@pytest.mark.parametrize("cid,Kd,k1,kernel", CONCAT, ids=[c[0] for c in CONCAT])
def test_fwd_epilogue_concat(K, dev, cid, Kd, k1, kernel, M, N, pro, stat_relu, pname):
    k2 = Kd - k1
    assert _route(N, Kd, k1, Kd, False, pro_a=pro, k1=k1, lda2=k2) == kernel
    g = torch.Generator().manual_seed(M + N + Kd + k1 + pro)
    A = torch.randn(M, k1, generator=g)
    A2 = torch.randn(M, k2, generator=g) - 0.5          # negative values a misplaced ReLU would clip
    W = torch.randn(N, Kd, generator=g) * Kd ** -0.5
    b = torch.randn(N, generator=g)
    s, t = torch.rand(k1, generator=g) + 0.5, torch.randn(k1, generator=g)
    kw = dict(pro_a=pro, pro_s=s.to(dev), pro_t=t.to(dev)) if pro else {}
    Y = torch.empty(M, N, device=dev)
    ws = torch.full((2, N, K.nblocks(M)), SENT, device=dev)
    K.gemm(M, N, Kd, A.to(dev), k1, W.to(dev), Kd, Y, N, epi=K.EPI_FWD, bias=b.to(dev), stat_ws=ws,
           stat_relu=stat_relu, A2=A2.to(dev), lda2=k2, k1=k1, **kw)
    ref = torch.cat([_pro(A, pro, s, t), A2.double()], 1) @ W.double().t() + b.double()
    _check_fwd(K, Y.cpu(), ws, ref, M, N, stat_relu, f"{cid} {pname}")


# Rows of A that are copies of one another give bitwise equal rows of Y (the same fma chain per
# element), scaled up so that the copied row is the column maximum in about a third of the columns
# and the minimum in another third. Copies in block 1: rows 130 / 138 / 162 (tile rows 2, 10, 34:
# one lane's own elements, r and i apart), 134 (the same wave's other lane half, lanes >= 32), 200
# (the other wave half); row 10 (block 0: across the blocks of the 256-row group 0); 300 / 400
# (blocks 2 and 3, group 1).
TIE_ROWS = [10, 130, 134, 138, 162, 200, 300, 400]


def pool_case(K, dev, N, group_rows, seed=0):
    """One EPI_FWD launch with pool_ws on M = 512 rows with forced ties -> (Y fp32 on the CPU,
    pool_ws on the device, float64 reference of Y)."""
    M, Kd = 512, 32
    g = torch.Generator().manual_seed(N + group_rows + seed)
    X = torch.randn(M, Kd, generator=g)
    X[TIE_ROWS] = 8.0 * X[TIE_ROWS[0]]
    W = torch.randn(N, Kd, generator=g) * Kd ** -0.5
    b = torch.randn(N, generator=g)
    R = torch.randn(M // 256, N, generator=g)
    Y = torch.empty(M, N, device=dev)
    ws = torch.full((2, N, K.nblocks(M)), SENT, device=dev)
    pw = torch.full((K.nblocks(M), 4, N), SENT, device=dev)
    kw = dict(rowbias=R.to(dev), ldr=N) if group_rows == 256 else {}     # rb_blk and the pool share group_rows
    K.gemm(M, N, Kd, X.to(dev), Kd, W.to(dev), Kd, Y, N, epi=K.EPI_FWD, bias=b.to(dev), stat_ws=ws,
           pool_ws=pw, group_rows=group_rows, **kw)
    ref = X.double() @ W.double().t() + b.double()
    if group_rows == 256:
        ref = ref + R[torch.arange(M) // 256].double()
    return Y.cpu(), pw, ref, ws


@pytest.mark.parametrize("N,kernel", [(192, "gemm2_tn2"), (40, "gemm2_tn1")])
@pytest.mark.parametrize("group_rows", [128, 256])
def test_fwd_pool_records(K, dev, N, kernel, group_rows):
    """pool_ws[blk] = {max, argmax, min, argmin} of the stored Y rows of block blk."""
    assert _route(N, 32, 32, 32, False) == kernel
    Y, pw, ref, ws = pool_case(K, dev, N, group_rows)
    _check_fwd(K, Y, ws, ref, 512, N, False, f"pool {kernel}")
    assert all(torch.equal(Y[130], Y[r]) for r in (134, 138, 162, 200))
    one = torch.ones(N)
    _, amax, vmax = bn_ref.pool_ref(Y, 128, one, 0 * one, False)       # per 128-row block, lowest row on ties
    _, amin, vmin = bn_ref.pool_ref(Y, 128, -one, 0 * one, False)
    rec = pw.cpu()
    reci = rec.view(torch.int32)
    assert torch.equal(rec[:, 0, :], vmax.float()), "block max"
    assert torch.equal(rec[:, 2, :], vmin.float()), "block min"
    assert torch.equal(reci[:, 1, :].long(), amax), "block argmax (lowest row on ties)"
    assert torch.equal(reci[:, 3, :].long(), amin), "block argmin (lowest row on ties)"
    # the ties are really there: in block 1 the copied row wins (as max or as min) in some
    # columns, at row 130 and not at its copies 134 / 138 / 162 / 200
    assert ((amax[1] == 130).sum() + (amin[1] == 130).sum()).item() >= N // 8
