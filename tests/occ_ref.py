"""numpy restatement of the partial-cloud generator (ured_occlude), written from its specification:
the counter-based random words, the plan draw, the four occlusion modes with float32 arithmetic in
the stated order, and centring / rotation in float64. Not a test; the tests import it.

Random words: word(seed, step, sample, stream, ctr) = output word 0 of Philox-4x32-10 with key
(seed low, seed high) and counter ((stream << 16) | ctr, sample, step low, step high).
Streams: 0 selection keys (ctr = point), 1 centre keys (ctr = point), 2 plan scalars (ctr 0 mode,
1 ncenter, 2 slice centre, 3-5 direction, 6 probe, 7-9 angles)."""
import numpy as np

M32 = 0xFFFFFFFF
BALL, RANDOM, SLICE, PART = 0, 1, 2, 3
F32 = np.float32


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) & np.uint64(M32) for c in counter]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        p0 = np.uint64(0xD2511F53) * c0          # < 2^64: both factors are below 2^32
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(M32),
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(M32))
    return c0, c1, c2, c3


def words(seed, step, sample, stream, ctr):
    """uint64 array (values below 2^32) of the words at counters `ctr` (array-like)."""
    ctr = np.asarray(ctr, np.uint64)
    assert (ctr < 65536).all() and 0 <= stream < 65536
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    z = np.zeros_like(ctr)
    c = (np.uint64(stream << 16) | ctr, z + np.uint64(sample), z + np.uint64(step & M32), z + np.uint64(step >> 32))
    return philox4x32_10(c, (seed & M32, seed >> 32))[0]


def unif(r):
    """(r >> 8) * 2^-24 as float32 (exact)."""
    return (np.asarray(r, np.uint64) >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)


def index(r, n):
    return int((int(r) * n) >> 32)


def draw_plan(seed, step, sample, N, mode=None):
    """-> dict(mode, ncenter, centres[8], slice_centre, probe, direction f32[3], angles f32[3])."""
    w = [int(v) for v in words(seed, step, sample, 2, np.arange(10))]
    u = unif(w[0])
    m = 0 if u < F32(0.3) else 1 if u < F32(0.6) else 2 if u < F32(0.9) else 3
    if mode is not None and mode >= 0:
        m = int(mode)
    ck = (words(seed, step, sample, 1, np.arange(N)) << np.uint64(32)) | np.arange(N, dtype=np.uint64)
    centres = np.argsort(ck, kind="stable")[:8]
    c = F32(1e-3) + unif(w[3:6]) * (F32(1.0) - F32(1e-3))
    nrm = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2], dtype=F32)
    return {"mode": m, "ncenter": 1 << index(w[1], 4), "centres": centres.astype(np.int64),
            "slice_centre": index(w[2], N), "probe": index(w[6], N), "direction": (c / nrm).astype(F32),
            "angles": (F32(-10.0) + F32(20.0) * unif(w[7:10])).astype(F32)}


def plan_arrays(plan):
    """(int32[12], float32[6]) in the device layout."""
    pi = np.array([plan["mode"], plan["ncenter"], *plan["centres"], plan["slice_centre"], plan["probe"]], np.int32)
    pf = np.concatenate([plan["direction"], plan["angles"]]).astype(F32)
    return pi, pf


def plan_from_arrays(pi, pf):
    return {"mode": int(pi[0]), "ncenter": int(pi[1]), "centres": np.asarray(pi[2:10], np.int64),
            "slice_centre": int(pi[10]), "probe": int(pi[11]), "direction": np.asarray(pf[:3], F32),
            "angles": np.asarray(pf[3:6], F32)}


def _smallest(hi, eligible, r0, m):
    """point indices at ranks [r0, r0+m) of the ascending keys (hi << 32) | index over the eligible."""
    idx = np.nonzero(eligible)[0].astype(np.uint64)
    keys = (np.asarray(hi, np.uint64)[idx.astype(np.int64)] << np.uint64(32)) | idx
    return (np.sort(keys)[r0:r0 + m] & np.uint64(M32)).astype(np.int64)


def _bits(f):
    f = np.ascontiguousarray(f, F32)
    assert not np.signbit(f).any()
    return f.view(np.uint32).astype(np.uint64)


def ball_survivors(x, plan):
    """bool [N]: not cancelled by any used centre (before the trim to K)."""
    x = np.asarray(x, F32)
    N = x.shape[0]
    cancel = (N // 2) // plan["ncenter"]
    alive = np.ones(N, bool)
    for c in plan["centres"][:plan["ncenter"]]:
        d = x - x[c]
        d = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        assert d.dtype == F32
        alive[_smallest(_bits(d), np.ones(N, bool), 0, cancel)] = False
    return alive


def select(x, sem, plan, seed, step, sample):
    """-> (ascending kept indices int64 [K], the branch taken)."""
    x = np.asarray(x, F32)
    N = x.shape[0]
    K = N // 2
    rnd = words(seed, step, sample, 0, np.arange(N))
    everyone = np.ones(N, bool)
    mode = plan["mode"]
    if mode == RANDOM:
        kept, branch = _smallest(rnd, everyone, 0, K), "random"
    elif mode == BALL:
        alive = ball_survivors(x, plan)
        assert alive.sum() >= K
        kept, branch = _smallest(rnd, alive, 0, K), "ball"
    elif mode == SLICE:
        d = x - x[plan["slice_centre"]]
        n = np.asarray(plan["direction"], F32)
        t = np.abs(((d[:, 0] * n[0]) + (d[:, 1] * n[1])) + (d[:, 2] * n[2]))
        assert t.dtype == F32
        kept, branch = _smallest(_bits(t), everyone, K - 1, K), "slice"
    elif mode == PART:
        surv = np.asarray(sem) != np.asarray(sem)[plan["probe"]]
        if surv.sum() > K:
            kept, branch = _smallest(rnd, surv, 0, K), "part-trim"
        else:
            kept, branch = _smallest(rnd, everyone, 0, K), "part-fallback"
    else:
        raise ValueError(mode)
    return np.sort(kept), branch


def rotation(angles_deg):
    """(Rx @ Ry @ Rz)[:3,:3] of the reference's rotation_matrix_3d, float64."""
    ax, ay, az = np.radians(np.asarray(angles_deg, np.float64))
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]], np.float64)
    ry = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]], np.float64)
    rz = np.array([[cz, sz, 0], [-sz, cz, 0], [0, 0, 1]], np.float64)
    return rx @ ry @ rz


def occlude_one(x, labels, sem, seed, step, sample, plan=None, mode=None, rotate=False):
    """One sample -> dict(mask, ori_point_occ, point_occ f64, labels_occ, sem_occ, occ_mean f64,
    occ_rot f64, plan, branch)."""
    x = np.asarray(x, F32)
    if plan is None:
        plan = draw_plan(seed, step, sample, x.shape[0], mode)
    mask, branch = select(x, sem, plan, seed, step, sample)
    ori = x[mask]
    mean = ori.astype(np.float64).mean(axis=0)
    R = rotation(plan["angles"]) if rotate else np.eye(3)
    p = (R @ (ori.astype(np.float64) - mean).T).T
    return {"mask": mask, "ori_point_occ": ori, "point_occ": p, "labels_occ": np.asarray(labels)[mask],
            "sem_occ": np.asarray(sem)[mask], "occ_mean": mean, "occ_rot": R, "plan": plan, "branch": branch}


def occlude(x, labels, sem, seed, step=0, modes=None, plans=None, rotate=False):
    """Batch form: list of occlude_one results (sample = position in the batch)."""
    out = []
    for b in range(len(x)):
        out.append(occlude_one(x[b], labels[b], sem[b], seed, step, b, plan=None if plans is None else plans[b],
                               mode=None if modes is None else modes[b], rotate=rotate))
    return out


def golden_slice_plan(g, i):
    """Plan of slice case i of tests/golden/occ.npz (g: the loaded arrays)."""
    return {"mode": SLICE, "ncenter": 1, "centres": np.zeros(8, np.int64), "slice_centre": int(g["slice_centre"][i]),
            "probe": 0, "direction": g["slice_direction"][i].astype(np.float32), "angles": np.zeros(3, np.float32)}


def golden_ball_plan(g, i):
    """Plan of ball case i of tests/golden/occ.npz (unused centre slots, -1 in the file, as 0)."""
    return {"mode": BALL, "ncenter": int(g["ball_ncenter"][i]), "centres": np.maximum(g["ball_centres"][i], 0),
            "slice_centre": 0, "probe": 0, "direction": np.array([1, 0, 0], np.float32), "angles": np.zeros(3, np.float32)}
