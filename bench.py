"""U-RED training-step benchmark on MI355X (BASELINE.json metric, config 2 by default).

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline line (value,
ms_per_step). --dump-outputs DIR also writes what the last timed step returned (and the model
state it left) as DIR/<name>.npy. Everything else the benchmark measures (the GEMM roofline and
per-variant breakdown, the all-slots / 16-part / loader rates, the chamfer, pseudo-label,
inference and EMD side measurements, the CPU baseline) runs only with --full.

N > 1: under torch.distributed.run (WORLD_SIZE set) each process is one rank; without it,
bench.py launches the N ranks itself (a torch.distributed.run child process, started before
anything touches the GPU) after checking that N GPUs are visible, and exits with its status.
n_gpus in the JSON line is dist.get_world_size().

A step = one full U-RED training iteration (engine/train.py:196-345): source +
target encoders, part pooling, 3 residual nets, DeformNet, get_shape, chamfer /
contrast / symmetry / residual / reconstruction losses, backward, 6x clip, Adam —
on a synthetic chair-shaped batch (bs=16 per GPU, 2048 points, 16 part slots x
1024 source points, C=512, S=128, 4 parts per target) resident in HBM.
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.add_pkg_path()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_FP32_TFLOPS = 157.3      # MI355X fp32 (vector = matrix) dense peak, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0
PMC_SUMMARY = "r6s_pmc_summary.json"   # FETCH/WRITE_SIZE passes of this default command (tools/gpu_prof.sh)
# rocprofv3 --kernel-trace --stats of the headline command (tools/prof_step.sh), restricted to its timed
# steps: the dominant kernel's average duration there is what roofline.achieved / frac are computed from
PROF_STATS = "r6s_step_kernel_stats.csv"
CLOCK_SUMMARY = "r6s_clock_summary.json"   # GRBM_GUI_ACTIVE pass (tools/gpu_clock_sq.sh): clock held per kernel
SQ_SUMMARY = "r6s_sq_summary.json"         # SQ pass (tools/gpu_clock_sq.sh): MFMA-busy cycles per kernel
NOMINAL_GHZ = 2.4


def workload_cfg(args):
    with open(os.path.join(ge.PKG_DIR, "config", "config_train_test.json")) as f:
        cfg = json.load(f)
    cfg.update({"batch_size": args.batch, "num_points": args.points, "parts": args.parts,
                "num_source": args.sources, "device": "cuda", "log_every": 0, "compute_connectivity": False,
                "flat_adam": os.environ.get("URED_FLAT_ADAM", "1") == "1",    # A/B knob: torch's Adam
                "loss_head": os.environ.get("URED_LOSS_HEAD", "1") == "1"})   # A/B knob: composed loss ops
    return cfg


def algo_bytes(M, N, K, epi):
    """Algorithmic HBM bytes of one launch: both operands once, the output once, plus the
    epilogue's read of the previous layer's output (BN backward)."""
    return 4.0 * (M * K + K * N + M * N) + (4.0 * M * N if epi == 2 else 0.0)


def variant_key(kw, M=None, N=None, K=None):
    """The kernel a kernels.gemm call launches (the name rocprof reports): the K <= 4 edge layers
    go to the streaming kernels (ured_gemm's fwd_small_ok / dgrad_small_ok), the rest to a
    gemm2_kernel template instance; None for an outer few-tile call that kernels.gemm splits
    into an EPI_SPLITK launch (+ reduce), which is timed on its own."""
    tf = {False: "false", True: "true"}
    ak, bk = bool(kw.get("a_kmajor", False)), bool(kw.get("b_kmajor", False))
    pa, pb, epi = kw.get("pro_a", 0), kw.get("pro_b", 0), kw.get("epi", 0)
    if K is not None:
        raw = pa == 0 and pb == 0 and not ak and kw.get("A2") is None and 1 <= K <= 4 and 1 <= N <= 256
        if raw and epi == 2 and bk and kw.get("pool_idx") is None:
            return f"dgrad_small_bnbwd_kernel<{K}>"
        if raw and epi == 1 and not bk and kw.get("pool_ws") is None and kw.get("rowbias") is None:
            return f"fwd_small_stats_kernel<{K}>"
        if (epi == 0 and pa == 0 and pb == 0 and kw.get("A2") is None and not ak and K >= 512
                and ((M + 127) // 128) * ((N + 127) // 128) <= 16):
            return None
    # block tile (csrc/mlp.hip launch()): 128 x 64 for <= 64 output columns, 64-row tiles for
    # split-K / store GEMMs of <= 64 rows (the instance's last two template arguments TM, TN)
    tn = 1 if N is not None and N <= 64 else 2
    tm = 1 if M is not None and M <= 64 and epi in (0, 3) else 2
    return f"gemm2_kernel<{tf[ak]}, {tf[bk]}, {pa}, {pb}, {epi}, {tm}, {tn}>"


class DominantTimer:
    """Inside the timed region: an event pair around every launch of ONE gemm variant (the
    dominant kernel), recorded on torch's current stream — the stream every ured launch uses."""

    def __init__(self, key):
        self.key, self.rec = key, []

    def __enter__(self):
        from ured_hip import kernels
        self.k, self.orig = kernels, kernels.gemm
        rec, key, orig = self.rec, self.key, self.orig

        def timed(M, N, K, *a, **kw):
            if variant_key(kw, M, N, K) != key:
                return orig(M, N, K, *a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            orig(M, N, K, *a, **kw)
            e1.record()
            rec.append((2.0 * M * N * K, algo_bytes(M, N, K, kw.get("epi", 0)), e0, e1))
        kernels.gemm = timed
        return self

    def __exit__(self, *exc):
        self.k.gemm = self.orig

    def summary(self):
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for _, _, e0, e1 in self.rec]
        # per-launch attainable time: max(FLOP / MFMA peak, algorithmic bytes / HBM peak)
        att = sum(max(f / (PEAK_FP32_TFLOPS * 1e12), b / (PEAK_HBM_GBS * 1e9)) for f, b, _, _ in self.rec) * 1e3
        return {"launches": len(ms), "ms": sum(ms), "flop": sum(r[0] for r in self.rec),
                "bytes": sum(r[1] for r in self.rec), "attainable_ms": att}


class GemmTimer:
    """Event pairs around every ured_gemm launch of one extra (untimed-region) step."""

    def __init__(self):
        self.rec = []

    def __enter__(self):
        from ured_hip import kernels
        self.k = kernels
        self.orig = kernels.gemm
        rec = self.rec

        def timed(M, N, K, *a, **kw):
            name = variant_key(kw, M, N, K)
            if name is None:        # split into an EPI_SPLITK launch (timed itself) + reduce
                return self.orig(M, N, K, *a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.orig(M, N, K, *a, **kw)
            e1.record()
            rec.append((name, kw.get("epi", 0), kw.get("a_kmajor", False), kw.get("b_kmajor", False),
                        kw.get("pro_a", 0), kw.get("pro_b", 0), int(M), int(N), int(K), e0, e1))
        kernels.gemm = timed
        return self

    def __exit__(self, *exc):
        self.k.gemm = self.orig

    def summary(self):
        torch.cuda.synchronize()
        by = {}
        for key, epi, ak, bk, pa, pb, M, N, K, e0, e1 in self.rec:
            ms = e0.elapsed_time(e1)
            d = by.setdefault(key, {"launches": 0, "ms": 0.0, "flop": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += ms
            d["flop"] += 2.0 * M * N * K
            d["bytes"] += algo_bytes(M, N, K, epi)
        return by

    def shapes(self, steps=1):
        torch.cuda.synchronize()
        by = {}
        for name, epi, ak, bk, pa, pb, M, N, K, e0, e1 in self.rec:
            key = f"{name.split('<')[0]} epi{epi} akm{int(bool(ak))} bkm{int(bool(bk))} pa{pa} pb{pb} M{M} N{N} K{K}"
            d = by.setdefault(key, {"launches": 0, "ms": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["tflops"] = round(2.0 * M * N * K * d["launches"] / (d["ms"] * 1e-3) / 1e12, 1)
        for d in by.values():   # per step
            d["launches"] /= steps
            d["ms"] /= steps
        return dict(sorted(by.items(), key=lambda kv: -kv[1]["ms"]))


def host_threads():
    """The host cores this process may use: its CPU affinity, capped by OMP_NUM_THREADS when set
    (the GPU box exports 16 = its CPU share; os.cpu_count() there is the whole machine's)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS")
    return max(1, min(n, int(omp))) if omp and omp.isdigit() else n


def _oracle_step_rate(cfg, batch_size, points, parts, sources, warm=1, timed=3):
    """1 warm-up + `timed` full oracle train steps (fwd + bwd + Adam, torch-CPU fp32) -> s/step."""
    from oracle import ured_ref
    from dataset import synthetic
    P = ured_ref.make_params(cfg, seed=0)
    for mod in P.values():
        for k, v in mod.items():
            if v.dtype.is_floating_point and "running" not in k:
                v.requires_grad_(True)
    db = synthetic.make_source_db(sources, seed=1)
    bt = synthetic.make_batch(batch_size, points, sources, parts=parts, seed=0)
    ob = {"src_points": torch.from_numpy(db["src_points"]), "src_mats": torch.from_numpy(db["src_mats"]),
          "src_sem": torch.from_numpy(db["src_sem"]), "src_index": torch.from_numpy(bt["src_index"]),
          "tgt_sem": torch.from_numpy(bt["tgt_sem"]), "x": torch.from_numpy(bt["x"]),
          "labels": torch.from_numpy(bt["labels"]).float(),
          "src_labels": torch.from_numpy(np.where(bt["src_labels"] >= 0, 1, bt["src_labels"]))}
    params = [v for _, _, v in ured_ref.trainable(P)]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=5e-4)
    ts = []
    for i in range(warm + timed):
        t0 = time.perf_counter()
        opt.zero_grad()
        loss, _ = ured_ref.train_forward(P, ob, cfg)
        loss.backward()
        opt.step()
        ts.append(time.perf_counter() - t0)
    return ts[warm:]


def _distchamfer_rate(B=16, n=2048, m=2048, reps=3):
    """The reference's Python chamfer (chamfer_python.distChamfer: float64 expansion matrix, min /
    argmin both ways), restated in the oracle -> Gpair-dist/s at 16 x 2048 x 2048."""
    from oracle import nn_ref
    g = torch.Generator().manual_seed(0)
    p1 = torch.rand(B, n, 3, generator=g)
    p2 = torch.rand(B, m, 3, generator=g)
    nn_ref.dist_chamfer(p1, p2)
    t0 = time.perf_counter()
    for _ in range(reps):
        nn_ref.dist_chamfer(p1, p2)
    t = (time.perf_counter() - t0) / reps
    return B * n * m / t / 1e9, t


def cpu_baseline(args):
    """The oracle (the CPU restatement of the reference's step, torch-CPU fp32) timed on this
    host, as BASELINE.md §2 plans: 1 warm-up + 3 timed full train steps at config 2 (the bench
    shape, 512 sources) and at config 1 (bs 2, 512 points), and the reference's Python chamfer
    (distChamfer) at 16 x 2048 x 2048 — all on host_threads() threads."""
    threads = host_threads()
    torch.set_num_threads(threads)
    cfg = workload_cfg(args)
    t2 = _oracle_step_rate(cfg, args.batch, args.points, args.parts, args.sources)
    cfg1 = dict(cfg, batch_size=2)
    t1 = _oracle_step_rate(cfg1, 2, 512, 4, args.sources)
    gp, tch = _distchamfer_rate()
    s2, s1 = sum(t2) / len(t2), sum(t1) / len(t1)
    return {"value": round(1.0 / s2, 5), "unit": "iters/s", "cores": threads, "kind": "port",
            "sample": f"oracle train step (fwd+bwd+Adam, torch-CPU fp32) at config 2 (bs={args.batch}, "
                      f"N={args.points}, {args.sources} sources, {args.parts} parts): 1 warm-up + {len(t2)} timed "
                      f"steps, {s2:.1f} s/step, on {threads} host threads",
            "config1_iters_s": round(1.0 / s1, 4),
            "config1_sample": f"config 1 (bs=2, N=512): 1 warm-up + {len(t1)} timed steps, {s1:.2f} s/step",
            "distchamfer_gpair_s": round(gp, 4),
            "distchamfer_sample": f"chamfer_python.distChamfer restated (float64 matrix), 16x2048x2048, {tch * 1e3:.0f} ms"}


def chamfer_rate(dev, B=16, n=2048, m=2048, iters=20):
    """NN forward (both directions) on one dense [B,n,3] x [B,m,3] call: Gpair-dist/s and the
    two SURVEY §8(d) roofline fractions (8 FLOP/pair vs 157.3 TFLOP/s FP32 VALU — the binding
    roof; 12 B/point read vs 8 TB/s HBM — the north star's, unattainable by construction).
    `ms` is the device time per call: `iters` calls captured in one HIP graph and replayed, so the
    Python / autograd / allocation cost of issuing each call (tens of µs on the host, the same
    order as the kernel at this size) is not in it; `ms_eager` times the same calls issued one by
    one from Python."""
    from ured_hip import nn as unn
    g = torch.Generator().manual_seed(0)
    p1 = torch.rand(B, n, 3, generator=g).to(dev)
    p2 = torch.rand(B, m, 3, generator=g).to(dev)
    for _ in range(3):
        unn.nn_dense(p1, p2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        unn.nn_dense(p1, p2)
    e1.record()
    torch.cuda.synchronize()
    t_eager = e0.elapsed_time(e1) / iters * 1e-3
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        unn.nn_dense(p1, p2)                 # warm the side stream's allocator pool
        with torch.cuda.graph(graph):
            for _ in range(iters):
                unn.nn_dense(p1, p2)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    reps = 5
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / (reps * iters) * 1e-3
    pairs = B * n * m
    return {"shape": f"{B}x{n}x{m}", "ms": round(t * 1e3, 4), "gpair_dist_s": round(pairs / t / 1e9, 1),
            "ms_eager": round(t_eager * 1e3, 4), "gpair_dist_s_eager": round(pairs / t_eager / 1e9, 1),
            "timing": f"{iters} calls in one HIP graph, replayed {reps}x",
            "path": "fused" if unn.use_fused(B, n, m) else "two-pass",
            "valu_frac": round(8 * pairs / t / 157.3e12, 4),
            "hbm_read_frac": round(12 * B * (n + m) / t / 8e12, 6)}


def chamfer_published_cmp(dev, iters=50):
    """BASELINE.md §1's only published hot-path number: chamfer3D forward+backward on
    p1 = 32x2000x3, p2 = 32x1000x3 in 1.4 ms (ChamferDistancePytorch/README.md:48-56, GPU model
    unstated). Same call through our drop-in chamfer_3DDist (allocation, both directions, the
    gradient of d1.mean() + d2.mean())."""
    from chamfer3D.dist_chamfer_3D import chamfer_3DDist
    cd = chamfer_3DDist()
    g = torch.Generator().manual_seed(0)
    p1 = torch.rand(32, 2000, 3, generator=g).to(dev).requires_grad_(True)
    p2 = torch.rand(32, 1000, 3, generator=g).to(dev).requires_grad_(True)

    def once():
        d1, d2, _, _ = cd(p1, p2)
        (d1.mean() + d2.mean()).backward()
    for _ in range(5):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / iters
    return {"shape": "32x2000x1000", "fwd_bwd_ms": round(t, 4), "gpair_s": round(32 * 2000 * 1000 / (t * 1e-3) / 1e9, 1),
            "published_ms": 1.4, "published_source": "ChamferDistancePytorch/README.md:48-56 (GPU unstated)",
            "speedup_vs_published": round(1.4 / t, 2)}


def emd_rate(dev, B=16, n=2048, eps=0.005, iters=50, reps=5):
    """§8(f)4: calc_emd's default auction (eps 0.005, 50 rounds, utils_v2/model_utils.py:72) on
    16 x 2048-point clouds: ms per call and the fraction of points matched one-to-one."""
    from emd import emd
    g = torch.Generator().manual_seed(0)
    x1 = torch.rand(B, n, 3, generator=g).to(dev)
    x2 = torch.rand(B, n, 3, generator=g).to(dev)
    m = emd()
    m(x1, x2, eps, iters)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dist, asg = m(x1, x2, eps, iters)
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / reps
    uniq = sum(int(torch.unique(asg[b]).numel()) for b in range(B)) / (B * n)
    return {"shape": f"{B}x{n}", "eps": eps, "rounds": iters, "ms": round(t, 3),
            "ms_per_round": round(t / max(iters, 1), 4),
            "bijective_fraction": round(uniq, 4), "emd": round(float(torch.sqrt(dist).mean()), 6)}


def inference_rate(cfg, db, dev, iters=30, reps=2):
    """Config 3 (table, bs=16, 2048 pts): the engine/test.py retrieval + deformation inference
    path — encode the source DB once (eval BN, chunks of 512), then per batch: target encoder,
    part pooling, cosine retrieval over the DB, DeformNet, get_shape, chamfer."""
    from engine.test import encode_sources, infer
    from engine.train import batch_to_device, get_models
    from dataset import synthetic
    models, _, _ = get_models(cfg, dev)
    b = batch_to_device(synthetic.make_batch(16, 2048, db.num_sources, parts=4, seed=77), dev, db.num_sources)
    codes = encode_sources(models, db)
    infer(models, db, b, cfg, codes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    codes = encode_sources(models, db)
    torch.cuda.synchronize()
    t_db = time.perf_counter() - t0
    # host-launch-bound (many small kernels per batch): best of `reps` timed runs
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            infer(models, db, b, cfg, codes)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e-3)
    t = min(ts)
    # the same path replayed as one HIP graph per batch shape (engine/test.py GraphedInfer)
    from engine.test import GraphedInfer
    gi = GraphedInfer(models, db, cfg, codes)
    gi(b)
    gi(b)
    torch.cuda.synchronize()
    tg = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            gi(b)
        e1.record()
        torch.cuda.synchronize()
        tg.append(e0.elapsed_time(e1) / iters * 1e-3)
    t_g = min(tg)
    return {"workload": "config 3: engine/test.py inference, bs=16, 2048 pts, 4 parts/target",
            "graph_batches_per_s": round(1.0 / t_g, 2), "graph_ms_per_batch": round(t_g * 1e3, 3),
            "runs_ms_per_batch": [round(x * 1e3, 3) for x in ts],
            "batches_per_s": round(1.0 / t, 2), "targets_per_s": round(16.0 / t, 1), "ms_per_batch": round(t * 1e3, 3),
            "source_db_encode_ms": round(t_db * 1e3, 3), "sources": int(db.num_sources)}


def pair_rate(dev, parts=512, pts=1024):
    """§8f row 1: all-pairs calc_dcd pseudo-labels over `parts` source parts (upper triangle)."""
    from engine.generate_pair import PairGenerator, normalize_pts
    from dataset import synthetic
    cl = np.stack([normalize_pts(p) for p in synthetic.make_source_db(parts, seed=1)["src_points"][:, :pts]])
    gen = PairGenerator(torch.from_numpy(cl).to(dev))
    gen.rows([0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gen.rows(range(parts))
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    npairs = parts * (parts + 1) // 2
    return {"parts": parts, "points": pts, "pairs": npairs, "seconds": round(t, 4),
            "pairs_per_s": round(npairs / t, 1), "gpair_dist_s": round(npairs * pts * pts / t / 1e9, 1)}


class GemmFlops:
    """Sum of 2MNK over the ured_gemm launches issued inside the context (no timing)."""

    def __enter__(self):
        from ured_hip import kernels
        self.k, self.orig, self.flop = kernels, kernels.gemm, 0.0

        def counted(M, N, K, *a, **kw):
            if variant_key(kw, M, N, K) is not None:     # the split-K store path counts once
                self.flop += 2.0 * M * N * K
            return self.orig(M, N, K, *a, **kw)
        kernels.gemm = counted
        return self

    def __exit__(self, *exc):
        self.k.gemm = self.orig


def batch_workload(eager, batch, num_sources):
    """(distinct source parts encoded, padded count, GEMM TFLOP) of one step on `batch` (one eager
    step outside any timed region)."""
    s = batch["src_unique"]
    with GemmFlops() as gf:
        eager.step(batch)
    return s.U_distinct, s.U, gf.flop / 1e12


def loader_rate(step, eager, cfg, db, dev, steps, world=1, rank=0, warm_epochs=2, head_batches=None):
    """The reference's per-iteration data path inside the timed loop (engine/train.py:190-232):
    every step takes its batch from engine/train.py's PseudoLabelLoader — a seeded shuffle of a
    fixed synthetic target set assembled from source parts (4 per target, as the headline), whose
    source labels the reference's get_labels rule picks on the device over a calc_dcd table
    (PseudoLabelTable) when the batch is drawn — copies the labels back to the host (as
    get_labels returns them), builds the batch's distinct-source tables there and uploads it from
    pinned host memory, then runs the same step as the headline (graph replay at N=1; the loader
    pads the distinct-source count to a multiple of 8 so that an epoch needs few graphs). Warm-up:
    whole epochs, so the graphs of the batch shapes an epoch produces are captured before timing.
    Reported beside the rate: the distinct source parts per step and the GEMM TFLOP per step of the
    loader's batches and of the headline's."""
    from engine.train import PseudoLabelLoader
    from train_utils.load_sources import source_connectivity
    dist_src = source_connectivity(db)[2]
    lcfg = dict(cfg, num_targets=max(128, 8 * cfg["batch_size"]), synthetic_targets="sources")
    ld = PseudoLabelLoader(lcfg, db, dev, dist_src, seed=17 + rank)

    def batches():
        while True:
            yield from ld
    it = batches()
    for _ in range(warm_epochs * len(ld)):
        step.step(next(it))
    graphs0 = getattr(step, "captures", 0)
    us, ups = [], []
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        bt = next(it)
        us.append(bt["src_unique"].U_distinct)
        ups.append(bt["src_unique"].U)
        step.step(bt)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    tt = torch.tensor([time.perf_counter() - t0], device=dev)
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    # the workload of both batch streams, outside the timed loop: one eager step per batch
    lw = [batch_workload(eager, next(it), db.num_sources) for _ in range(4)]
    hw = [batch_workload(eager, b, db.num_sources) for b in (head_batches or [])]
    mean = lambda v: round(float(np.mean(v)), 2) if v else None      # noqa: E731
    return {"iters_s": round(steps * world / float(tt.item()), 4), "steps": steps,
            "graphs_captured_in_timed_steps": getattr(step, "captures", 0) - graphs0,
            "num_targets": lcfg["num_targets"],
            "distinct_sources_per_step": mean(us), "padded_sources_per_step": mean(ups),
            "gemm_tflop_per_step": mean([w[2] for w in lw]),
            "headline_distinct_sources_per_step": mean([w[0] for w in hw]),
            "headline_padded_sources_per_step": mean([w[1] for w in hw]),
            "headline_gemm_tflop_per_step": mean([w[2] for w in hw]),
            "what": "each step: PseudoLabelLoader batch (targets assembled from source parts, 4 per target; the "
                    "get_labels rule evaluated on the device over a calc_dcd table when the batch is drawn, labels "
                    "copied to the host, host distinct-source tables) + pinned-memory upload inside the timed loop"}


DUMP_BUDGET_BYTES = 60 << 20      # --dump-outputs writes at most this much (the limit is 64 MB)


def snapshot_outputs(T, step):
    """What a caller of the timed path holds after its last step, copied to the host: the step's
    returned dict (the loss terms, the deformed shapes `_out`, the deformation parameters
    `_params`) as out.<key>, and the state the step left in the models as state.<module>.<key>.
    float32 stays float32, every other dtype becomes float64."""
    torch.cuda.synchronize()
    arrs = {}

    def put(name, v):
        v = v.detach().cpu()
        arrs[name] = v.numpy().astype(np.float32 if v.dtype == torch.float32 else np.float64)
    for k, v in T.items():
        if torch.is_tensor(v):
            put("out." + k.lstrip("_"), v)
    for mod, sd in step.state_dict().items():
        for k, v in sd.items():
            put(f"state.{mod}.{k}", v)
    return arrs


def dump_outputs(arrs, out_dir):
    """DIR/<name>.npy, DUMP_BUDGET_BYTES in all: the arrays share the budget smallest first, and one
    that exceeds its share is written as a fixed sample of its flattened elements (sorted indices
    drawn by a generator seeded with the array's name and size, the same in every run)."""
    import zlib
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BUDGET_BYTES
    names = sorted(arrs, key=lambda n: (arrs[n].nbytes, n))
    for i, name in enumerate(names):
        a = arrs[name]
        share = left // (len(names) - i)
        if a.nbytes > share:
            n = max(1, share // a.itemsize)
            rng = np.random.default_rng([zlib.crc32(name.encode()), a.size])
            a = a.reshape(-1)[np.sort(rng.choice(a.size, size=n, replace=False))]
        left -= a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)


def _free_port():
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    return port


def launch_ranks(args):
    """`--gpus N` without torch.distributed.run: start the N ranks as a child process (nothing in
    this process has initialised the GPU: torch.cuda.device_count() does not on this image)."""
    if not args.cpu_dry_run and args.dist_backend == "nccl":
        n = torch.cuda.device_count()
        if n < args.gpus:
            print(f"bench.py: --gpus {args.gpus} but only {n} GPU(s) visible", file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"))
    return subprocess.call(cmd, env=env)


def dry_run(args):
    """--cpu-dry-run: the launcher and the rank bookkeeping of the JSON line without a GPU (gloo;
    each "step" is an all_reduce of a 1 M-float buffer). For the CPU tests only."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo")
        world = dist.get_world_size()
    rank = dist.get_rank() if world > 1 else 0
    buf = torch.ones(1 << 20)
    for _ in range(args.warmup):
        if world > 1:
            dist.all_reduce(buf)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if world > 1:
            dist.all_reduce(buf)
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        el = float(t.item())
        print(json.dumps({"metric": "cpu dry run (launcher check, no GPU work)", "value": args.steps * world / el,
                          "unit": "iters/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": el / args.steps * 1e3, "dry_run": True}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # 50 timed steps after 8 warmup steps (the 4 batches' graphs captured, then each replayed once):
    # the steady-state rate; a 10-step window right after the captures read 2 % low
    # (profiles/r5s_bench_window.log)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--sources", type=int, default=512)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one returned and the model state it left "
                         "as DIR/<name>.npy (float32 / float64, at most 64 MB; larger arrays as a fixed sample)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: GEMM roofline and breakdown, the all-slots, "
                         "16-part and loader rates, the chamfer / pseudo-label / inference / EMD side measurements "
                         "and the CPU baseline (each can be switched off by its --no-* option)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--breakdown-steps", type=int, default=3, help="eager steps timed per GEMM launch after the run")
    ap.add_argument("--shapes-out", default=None,
                    help="write the per-shape GEMM breakdown (JSON) here (part of the --full breakdown)")
    ap.add_argument("--eager", action="store_true",
                    help="issue the step eagerly (Python + ctypes launches, ~700 per step) instead of replaying it "
                         "as HIP graphs. Graph replay (engine/graph.py, bitwise equal to eager) is the default at "
                         "N=1: the GPU-side step is ~16 ms, and on a slow host the eager launch stream cannot keep "
                         "up (51 vs 63 it/s measured on one box). N > 1 replays too: the captured step is split "
                         "at its collectives, which run eagerly between the graph segments (engine/graph.py)")
    ap.add_argument("--graph", action="store_true", help=argparse.SUPPRESS)   # the default; kept for old commands
    ap.add_argument("--graph-dp", action="store_true", help=argparse.SUPPRESS)   # graph replay is the N > 1 default
    ap.add_argument("--graph-bucket", type=int, default=1,
                    help="graph mode: pad the distinct-source-part count to a multiple of this (one graph per count)")
    ap.add_argument("--all-slots", action="store_true",
                    help="encode every source slot (no unique-source encoding) in the timed run")
    ap.add_argument("--blas", choices=["default", "hipblaslt", "rocblas"], default="rocblas",
                    help="torch matmul backend for the small DeformNet / contrast GEMMs")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the chamfer / pseudo-label side measurements (step-only profiles)")
    ap.add_argument("--no-all-slots-rate", action="store_true",
                    help="skip the extra timed run that encodes every source slot")
    ap.add_argument("--no-k16-rate", action="store_true",
                    help="skip the extra timed run at 16 parts per target (no padding slots)")
    ap.add_argument("--no-loader-rate", action="store_true",
                    help="skip the extra timed run that takes every batch from the pseudo-label loader "
                         "and uploads it inside the timed loop")
    ap.add_argument("--cpu-dry-run", action="store_true", help=argparse.SUPPRESS)
    # gloo: every rank on GPU (local rank mod the device count) — the rehearsal of the N > 1 code
    # path on a one-GPU box (tests); its rates mean nothing
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.full:       # a plain run: the headline only
        args.no_cpu_baseline = args.no_breakdown = args.no_extras = True
        args.no_all_slots_rate = args.no_k16_rate = args.no_loader_rate = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    if args.cpu_dry_run:
        return dry_run(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        if args.dist_backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            local %= torch.cuda.device_count()
            torch.cuda.set_device(local)
            dist.init_process_group("gloo")
        world, rank = dist.get_world_size(), dist.get_rank()
    if world != args.gpus and rank == 0:
        print(f"bench.py: running {world} rank(s) (--gpus {args.gpus})", file=sys.stderr)
    dev = torch.device("cuda", local)
    torch.manual_seed(1234 + rank)

    ge.build()
    if args.blas != "default":
        torch.backends.cuda.preferred_blas_library("cublaslt" if args.blas == "hipblaslt" else "cublas")
    from engine.dp import DataParallelStep
    from engine.train import batch_to_device
    from train_utils.load_sources import load_sources
    from dataset import synthetic

    cfg = workload_cfg(args)
    use_graph = not args.eager
    cfg["cuda_graph"] = use_graph
    db, _ = load_sources(cfg, dev)
    eager = DataParallelStep(cfg, db, dev)
    cfg["unique_sources"] = not args.all_slots
    batches = [batch_to_device(synthetic.make_batch(args.batch, args.points, db.num_sources, parts=args.parts,
                                                    seed=1000 * rank + i), dev, db.num_sources,
                               bucket=args.graph_bucket if use_graph else None) for i in range(4)]
    if use_graph:   # one graph per padded distinct-part count, captured after that batch's eager step
        from engine.graph import GraphedStep
        step = GraphedStep(eager)
        args.warmup = max(args.warmup, len(batches))   # every batch's graph is captured before timing
    else:
        step = eager

    b0 = None
    if use_graph and args.full:
        # the dominant GEMM variant's launches / FLOPs / bytes per step (for the roofline) from one
        # eager step with an event pair per GEMM launch, before the graphs are captured; one plain
        # eager step first, so that no kernel's first launch (code-object load) is among them
        eager.step(batches[0])
        with GemmTimer() as gt0:
            eager.step(batches[0])
        b0 = gt0.summary()
    for i in range(args.warmup):
        step.step(batches[i % 4])
    # one more untimed step with an event pair per GEMM launch picks the dominant kernel
    # variant, whose launches are then timed inside the timed region itself (eager mode)
    dom = None
    if not use_graph and args.full:
        with GemmTimer() as gt0:
            eager.step(batches[args.warmup % 4])
        b0 = gt0.summary()
        dom = DominantTimer(max(b0, key=lambda k: b0[k]["ms"]))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if dom is not None:
        dom.__enter__()
    for i in range(args.steps):
        T = step.step(batches[i % 4])
    if dom is not None:
        dom.__exit__(None, None, None)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    loss_val = float(T["all_loss"].item())
    if args.dump_outputs and rank == 0:      # before any --full side run trains the models further
        dump_outputs(snapshot_outputs(T, step), args.dump_outputs)

    def timed_rate(steps, bs=None):
        """A side workload under the headline's protocol: the same step mode (HIP-graph replay
        unless --eager, each batch's graph captured and replayed once before timing, in a
        GraphedStep of its own so the headline's graphs stay as they are), barrier + sync on both
        sides, max over ranks. So a side rate differs from the headline by its workload alone."""
        bs = bs or batches
        runner = eager
        warm = 2
        if use_graph:
            from engine.graph import GraphedStep
            runner = GraphedStep(eager, max_graphs=len(bs))
            warm = 2 * len(bs)
        for i in range(warm):
            runner.step(bs[i % len(bs)])
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t1 = time.perf_counter()
        for i in range(steps):
            runner.step(bs[i % len(bs)])
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        tt = torch.tensor([time.perf_counter() - t1], device=dev)
        if world > 1:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        if runner is not eager:           # release the side workload's graphs and their pools
            runner.graphs.clear()
            runner.g_update = None
            del runner
            import gc
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
        return steps * world / float(tt.item())

    all_slots_rate = None
    if not args.no_all_slots_rate and cfg["unique_sources"]:
        cfg["unique_sources"] = False      # every one of the B x 16 source slots encoded
        all_slots_rate = timed_rate(args.steps)
        cfg["unique_sources"] = True
    loader = None
    if not args.no_loader_rate and not args.no_extras:
        loader = loader_rate(step, eager, dict(cfg, unique_sources=True), db, dev, args.steps, world, rank,
                             head_batches=batches)
    k16_rate = None
    if not args.no_k16_rate and args.parts != 16:
        # SURVEY §8(d)'s stress case: 16 parts per target, no padding slots (~200 distinct sources)
        b16 = [batch_to_device(synthetic.make_batch(args.batch, args.points, db.num_sources, parts=16,
                                                    seed=5000 + 1000 * rank + i), dev, db.num_sources,
                               bucket=args.graph_bucket if use_graph else None)
               for i in range(4)]
        k16_rate = timed_rate(args.steps, b16)
        del b16

    breakdown = None
    if not args.no_breakdown:
        with GemmTimer() as gt:   # eager steps (same kernels) with per-launch events
            for i in range(args.breakdown_steps):
                eager.step(batches[i % 4])
        breakdown = gt.summary()
        for v in breakdown.values():   # per-step figures
            for k in ("launches", "ms", "flop", "bytes"):
                v[k] /= args.breakdown_steps
        if args.shapes_out and rank == 0:
            with open(args.shapes_out, "w") as f:
                json.dump(gt.shapes(args.breakdown_steps), f, indent=1)

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    ms = elapsed / args.steps * 1e3
    iters_per_s = args.steps / elapsed
    roofline = None
    extra = {}
    if breakdown or dom is not None or b0:
        if dom is not None:     # measured inside the timed region
            dom_key = dom.key
            d = dom.summary()
            timing = "HIP events around each launch of this kernel inside the timed region"
            lps = d["launches"] / args.steps
        else:                   # graph replay: per-launch events from eager steps outside it
            src = breakdown if breakdown else b0
            dom_key = max(src, key=lambda k: src[k]["ms"])
            d = src[dom_key]
            timing = ("HIP events around each launch in separate eager steps after the timed region" if breakdown
                      else "HIP events around each launch in one eager step before the timed region")
            lps = d["launches"]
        avg_ms = d["ms"] / d["launches"]
        flop_per_launch = d["flop"] / d["launches"]
        ach = flop_per_launch / (avg_ms * 1e-3) / 1e12
        live = {"avg_launch_ms": round(avg_ms, 4), "achieved": round(ach, 2),
                "frac": round(ach / PEAK_FP32_TFLOPS, 4), "timing": timing}
        # primary figures: the committed rocprof kernel-trace average of this kernel (same command,
        # timed steps); the profiler lengthens in-step kernels by a few %, so the live
        # HIP-event figures are reported beside them
        prof = os.path.join(ROOT, "profiles", PROF_STATS)
        prof_avg = None
        if os.path.exists(prof):
            import csv
            with open(prof) as f:
                for row in csv.DictReader(f):
                    if dom_key in row["Name"]:
                        prof_avg = float(row["AverageNs"]) * 1e-6
        # the committed trace is of the default workload: a run of another size (e.g. the tests' small
        # --batch) keeps its live figures (a >25 % mismatch with them marks another workload)
        if prof_avg and abs(prof_avg / avg_ms - 1.0) > 0.25:
            prof_avg = None
        if prof_avg:
            avg_ms, ach = prof_avg, flop_per_launch / (prof_avg * 1e-3) / 1e12
            timing = (f"rocprofv3 kernel-trace average of this kernel over the timed steps of the same command "
                      f"({os.path.relpath(prof, ROOT)})")
        traffic, tsrc = None, None
        profiled = prof_avg is not None      # the profile files describe this run's workload
        pmc = os.path.join(ROOT, "profiles", PMC_SUMMARY)
        if profiled and os.path.exists(pmc):
            pm = json.load(open(pmc))
            for kname, v in pm.items():
                if dom_key in kname:
                    traffic, tsrc = v["hbm_bytes_per_launch"], os.path.relpath(pmc, ROOT)
        roofline = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach / PEAK_FP32_TFLOPS, 4),
                    "traffic": None if traffic is None else round(traffic), "traffic_source": tsrc,
                    "algorithmic_bytes_per_launch": round(d["bytes"] / d["launches"]),
                    "kernel": dom_key, "launches_per_step": round(lps, 2), "avg_launch_ms": round(avg_ms, 4),
                    "flop_per_launch": round(flop_per_launch), "timing": timing, "live_hip_events": live}
        clk = os.path.join(ROOT, "profiles", CLOCK_SUMMARY)
        if profiled and os.path.exists(clk):
            for kname, v in json.load(open(clk)).items():
                if dom_key in kname:
                    # the chip holds ~2.2 GHz under this MFMA load (DVFS): the peak at that clock
                    ghz = v["effective_ghz"]
                    roofline["held_clock_ghz"] = round(ghz, 3)
                    roofline["frac_at_held_clock"] = round(ach / (PEAK_FP32_TFLOPS * ghz / NOMINAL_GHZ), 4)
                    roofline["clock_source"] = os.path.relpath(clk, ROOT)
        sq = os.path.join(ROOT, "profiles", SQ_SUMMARY)
        if profiled and os.path.exists(sq):
            for kname, v in json.load(open(sq)).items():
                if dom_key in kname and v.get("GRBM_GUI_ACTIVE"):
                    # SQ_VALU_MFMA_BUSY_CYCLES over the 1024 SIMDs x the kernel's cycles
                    roofline["mfma_busy"] = round(v["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024 * v["GRBM_GUI_ACTIVE"] / 8), 4)
        if "attainable_ms" in d:
            # the same launches against the per-launch roofline min(MFMA peak, AI x HBM peak): the
            # small-K shapes of this kernel sit near the ridge (AI ~ 20-40 FLOP/B)
            att_tf = d["flop"] / (d["attainable_ms"] * 1e-3) / 1e12
            roofline["attainable_tflops"] = round(att_tf, 2)
            roofline["frac_of_attainable"] = round(ach / att_tf, 4)
    if breakdown:
        tot_ms = sum(v["ms"] for v in breakdown.values())
        tot_flop = sum(v["flop"] for v in breakdown.values())
        extra["gemm_all"] = {"ms_per_step": round(tot_ms, 3), "tflop_per_step": round(tot_flop / 1e12, 4),
                             "tflops": round(tot_flop / (tot_ms * 1e-3) / 1e12, 2)}
        extra["gemm_variants"] = {k: {"launches": round(v["launches"], 2), "ms": round(v["ms"], 3),
                                      "tflops": round(v["flop"] / max(v["ms"], 1e-9) / 1e9, 2)}
                                  for k, v in sorted(breakdown.items(), key=lambda kv: -kv[1]["ms"])}
    if all_slots_rate is not None:
        extra["all_slots_iters_s"] = round(all_slots_rate, 4)
    if k16_rate is not None:
        extra["k16_iters_s"] = round(k16_rate, 4)
    if all_slots_rate is not None or k16_rate is not None:
        extra["side_rates_mode"] = "hip_graph" if use_graph else "eager"
    if loader is not None:
        extra["loader_iters_s"] = loader["iters_s"]
        extra["loader"] = loader
    extra["unique_sources"] = bool(cfg["unique_sources"])
    red = getattr(eager, "reducer", None)
    if world > 1 and red is not None:
        # gradient buckets all-reduced between the captured backward's segments; hooks that ran off
        # the capture stream leave their bucket to the end of the backward (engine/dp.py)
        extra["dp_overlap"] = {"buckets": red.num_buckets, "deferred_hooks": len(red.deferred),
                               "deferred_sample": red.deferred[:4]}
    if not args.no_extras:
        ch = chamfer_rate(dev)
        extra["chamfer_gpair_s"] = ch["gpair_dist_s"]
        extra["chamfer"] = [ch, chamfer_rate(dev, 64, 4096, 4096, iters=10),
                            chamfer_rate(dev, 16, 16384, 2048, iters=10)]
        extra["chamfer_vs_published"] = chamfer_published_cmp(dev)
        extra["pseudo_label_dcd"] = pair_rate(dev)
        extra["inference"] = inference_rate(cfg, db, dev)
        extra["emd"] = emd_rate(dev)
    extra["loss"] = loss_val
    cpu = None if (args.no_cpu_baseline or world > 1) else cpu_baseline(args)   # rank 0 at N=1 only
    out = {"metric": "train iters/sec chair bs=16 2048-pt @1/2/4/8 GPU; Chamfer Gpair-dist/s",
           "value": round(iters_per_s * world, 4), "unit": "iters/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
           "step_mode": "hip_graph" if use_graph else "eager", "full": bool(args.full),
           "vs_baseline": None, "dtype": "f32", "data": "synthetic (SURVEY §8d generator; random-init weights)",
           "config": {"workload": "config 2: chair, full U-RED train step, bs=16/GPU, 2048 pts, 16x1024 source pts, "
                                  "C=512, S=128, 4 parts/target", "global_batch": args.batch * world,
                      "points": args.points, "parallelism": f"dp{world}",
                      "samples_per_s": round(iters_per_s * world * args.batch, 2)},
           "roofline": roofline, "cpu_baseline": cpu}
    out.update(extra)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
