"""Float64 restatement of the optimizer tail (ured_adam_clip_step, csrc/optim.hip; contract in
include/ured_hip.h) and a builder of its chunk tables, shared by tests/test_optim_gpu.py. Plain numpy
on the CPU. tests/test_optim_ref.py pins adam_clip_step_ref to torch.nn.utils.clip_grad_norm_ per
module followed by torch.optim.Adam in float64, and chunk_tables to the header's contract and to
FlatAdam._set_active, so the GPU tests compare the kernels with arithmetic and tables that have an
independent check of their own.

The operation (reference engine/train.py:331-346, train_utils/optimizer_dm.py:68-104): per module
segment, the L2 norm over the gradients of the parameters that have one this step and
coef = min(max_norm / (norm + 1e-6), 1) (nan when the norm is nan: torch's clamp propagates it;
1 when max_norm <= 0); then, for those parameters only, one more step on the parameter's own step
count t and
    g *= coef;  g' = g + wd*p;  m = b1*m + (1-b1)*g';  v = b2*v + (1-b2)*g'^2
    p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
A parameter without a gradient is returned untouched: no decay of p, m or v, no step.
"""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
CHUNK = 8192                # elements per workgroup of the three kernels
ALIGN = 16                  # floats; every parameter slice starts on a multiple of it
LT = 256                    # threads per workgroup


def _f64(a):
    return np.array(a, dtype=np.float64, copy=True).reshape(-1)


def segment_norms(g, seg_of, active, nseg):
    """float64 L2 norm per segment over the active parameters' gradients (0 for an empty one)."""
    sq = np.zeros(nseg)
    for gi, s, a in zip(g, seg_of, active):
        if a:
            x = np.asarray(gi, dtype=np.float64).reshape(-1)
            with np.errstate(over="ignore", invalid="ignore"):
                sq[s] += np.sum(x * x)
    return np.sqrt(sq)


def clip_coefs(norm, max_norm):
    """coef = min(max_norm / (norm + 1e-6), 1) with torch's clamp semantics (nan stays nan)."""
    norm = np.asarray(norm, dtype=np.float64)
    if max_norm <= 0:
        return np.ones_like(norm)
    c = max_norm / (norm + 1e-6)
    return np.where(c > 1.0, 1.0, c)             # nan > 1 is False: nan propagates; inf norm -> 0


def adam_clip_step_ref(p, g, m, v, step, seg_of, active, max_norm, lr, b1, b2, eps, wd, coef=None, nseg=None):
    """One clip + Adam step on per-parameter arrays (lists, one entry per parameter; widened to
    float64 and copied, the inputs are left alone). step: per-parameter counts before this step.
    coef: per-segment coefficients to use instead of the computed ones (e.g. the GPU's).
    -> dict(p, g, m, v: lists of float64 arrays; step; coef; norm)."""
    n = len(p)
    nseg = (max(seg_of) + 1 if n else 1) if nseg is None else nseg
    P, G, M, V = ([_f64(x) for x in t] for t in (p, g, m, v))
    step = np.array(step, dtype=np.float64, copy=True)
    norm = segment_norms(G, seg_of, active, nseg)
    used = clip_coefs(norm, max_norm) if coef is None else np.asarray(coef, dtype=np.float64)
    assert used.shape == (nseg,)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            if not active[i]:
                continue
            step[i] += 1.0
            t = step[i]
            G[i] = G[i] * used[seg_of[i]]
            gw = G[i] + wd * P[i]
            M[i] = b1 * M[i] + (1.0 - b1) * gw
            V[i] = b2 * V[i] + (1.0 - b2) * gw * gw
            denom = np.sqrt(V[i]) / np.sqrt(1.0 - b2 ** t) + eps
            P[i] = P[i] - lr / (1.0 - b1 ** t) * M[i] / denom
    return dict(p=P, g=G, m=M, v=V, step=step, coef=used, norm=norm)


def chunk_tables(sizes, seg_of, active, chunk=CHUNK, align=ALIGN, offsets=None, nseg=None):
    """The tables ured_adam_clip_step takes, from the contract in include/ured_hip.h: parameter i
    (sizes[i] elements, module segment seg_of[i]) owns the slice [offsets[i], offsets[i] + sizes[i])
    of the flat buffers, padded with zeros to a multiple of `align`; by default the slices follow
    one another in index order. Only active parameters are listed; their padded slices are cut into
    chunks of at most `chunk` elements, segment-major (each segment's chunks contiguous, parameters
    in index order inside a segment).
    -> dict(chunk_beg, chunk_end int64; chunk_seg, chunk_param, seg_chunk0 [nseg + 1],
            active_params int32; offsets, total, nseg)."""
    assert chunk % align == 0 and align % 4 == 0
    n = len(sizes)
    nseg = (max(seg_of) + 1 if n else 1) if nseg is None else nseg
    pad = [-(-s // align) * align for s in sizes]
    if offsets is None:
        offsets = [int(x) for x in np.cumsum([0] + pad[:-1])] if n else []
    offsets = [int(o) for o in offsets]
    total = max([o + q for o, q in zip(offsets, pad)], default=0)
    cb, ce, cs, cp, s0 = [], [], [], [], [0]
    for s in range(nseg):
        for i in range(n):
            if seg_of[i] != s or not active[i]:
                continue
            end = offsets[i] + pad[i]
            b = offsets[i]
            while b < end:
                cb.append(b)
                ce.append(min(b + chunk, end))
                cs.append(s)
                cp.append(i)
                b += chunk
        s0.append(len(cb))
    return dict(chunk_beg=np.array(cb, dtype=np.int64), chunk_end=np.array(ce, dtype=np.int64),
                chunk_seg=np.array(cs, dtype=np.int32), chunk_param=np.array(cp, dtype=np.int32),
                seg_chunk0=np.array(s0, dtype=np.int32),
                active_params=np.array([i for i in range(n) if active[i]], dtype=np.int32),
                offsets=offsets, total=int(total), nseg=nseg)
