"""ured_occlude (csrc/occ.hip: partial target clouds in one launch) against the numpy oracle
tests/occ_ref.py and the reference's own gen_occ_point.py (tests/golden/occ.npz).

mask / labels_occ / sem_occ / ori_point_occ are compared bit for bit with the oracle run on the
plan the device returned (its float fields are fed to the oracle, so the comparison does not hinge
on sqrt / sin / cos rounding); the drawn plan itself is compared separately. point_occ, occ_mean
and occ_rot are compared with the float64 oracle at atol 2e-6 for coordinates in [-1, 1] (one
rounding of an fp64 mean, one subtraction, a 3x3 product: each ~1e-7)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import occ_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ATOL = 2e-6
MAX_ERR = {"v": 0.0}


@pytest.fixture(autouse=True)
def _occ_debug_word():
    """The debug build's bounds word of occ.hip (file id 11), read and cleared after each test."""
    yield
    mod = sys.modules.get("ured_hip._lib")
    if mod is None or mod._lib is None or not hasattr(mod._lib, "ured_dbg_occ"):
        return
    fn = mod._lib.ured_dbg_occ
    fn.restype, fn.argtypes = ctypes.c_ulonglong, [ctypes.c_int]
    torch.cuda.synchronize()
    v = fn(1)
    assert not v, f"device-side bounds check violated (debug build): occ.hip:{v & 0xFFFFFFFF}"


def cloud(B, N, seed, nsem=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-1, 1, size=(B, N, 3)).astype(np.float32)
    return x, rng.integers(0, 6, size=(B, N)), rng.integers(0, nsem, size=(B, N))


def run(dev, x, lab, sem, seed, step=0, modes=None, plans=None, rotate=False):
    from ured_hip import occ
    plan = None
    if plans is not None:
        pi, pf = zip(*[occ_ref.plan_arrays(p) for p in plans])
        plan = (torch.from_numpy(np.stack(pi)).to(dev), torch.from_numpy(np.stack(pf)).to(dev))
    r = occ.occlude(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(sem).to(dev),
                    seed, step, modes=modes, plan=plan, rotate=rotate)
    return {k: v.cpu().numpy() for k, v in r.items()}


def check(r, x, lab, sem, seed, step, rotate):
    """device result == oracle on the device's plan; -> the oracle's results."""
    out = []
    for b in range(len(x)):
        plan = occ_ref.plan_from_arrays(r["plan_i"][b], r["plan_f"][b])
        o = occ_ref.occlude_one(x[b], lab[b], sem[b], seed, step, b, plan=plan, rotate=rotate)
        assert np.array_equal(r["mask"][b], o["mask"]), (b, plan)
        assert np.array_equal(r["labels_occ"][b], o["labels_occ"]) and np.array_equal(r["sem_occ"][b], o["sem_occ"])
        assert np.array_equal(r["ori_point_occ"][b].view(np.uint32), o["ori_point_occ"].view(np.uint32))
        err = max(np.abs(r[k][b] - o[k]).max() for k in ("point_occ", "occ_mean", "occ_rot"))
        MAX_ERR["v"] = max(MAX_ERR["v"], float(err))
        print(f"occ max |err| vs float64 oracle: sample {b} {err:.3e} (running max {MAX_ERR['v']:.3e})")
        assert err <= ATOL, (b, err)
        if not rotate:
            assert np.array_equal(r["occ_rot"][b], np.eye(3, dtype=np.float32))
        out.append(o)
    return out


def check_drawn(r, seed, step, N, modes=None):
    for b in range(len(r["plan_i"])):
        pi, pf = occ_ref.plan_arrays(occ_ref.draw_plan(seed, step, b, N, None if modes is None else modes[b]))
        assert np.array_equal(r["plan_i"][b], pi), (b, r["plan_i"][b], pi)
        assert np.abs(r["plan_f"][b] - pf).max() <= 1e-6


# 16 and 100 sort inside one wave; 300 / 600 / 1000 pad to 512 / 1024 keys (several waves, one
# pair per thread); 2048 is the reference's size; 4096 and 3000 pad to 4096 (two pairs per thread,
# 3-4 points per thread in the scan)
SIZES = [16, 100, 300, 600, 1000, 2048, 3000, 4096]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_forced_modes(dev, B, N, mode):
    x, lab, sem = cloud(B, N, 1000 * N + 10 * B + mode)
    seed, step = 0x1234567890ABCDEF + N, (3 << 32) | B
    r = run(dev, x, lab, sem, seed, step, modes=[mode] * B, rotate=True)
    assert (r["plan_i"][:, 0] == mode).all()
    check_drawn(r, seed, step, N, [mode] * B)
    check(r, x, lab, sem, seed, step, True)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("ncenter", [1, 2, 4, 8])
def test_ball_with_each_centre_count(dev, B, N, ncenter):
    x, lab, sem = cloud(B, N, 77 * N + B + ncenter)
    seed, step = 99 + ncenter, N
    plans = [dict(occ_ref.draw_plan(seed, step, b, N, occ_ref.BALL), ncenter=ncenter) for b in range(B)]
    r = run(dev, x, lab, sem, seed, step, plans=plans, rotate=(B == 5))
    for b in range(B):                                 # the given plan is the plan used
        pi, pf = occ_ref.plan_arrays(plans[b])
        assert np.array_equal(r["plan_i"][b], pi) and np.array_equal(r["plan_f"][b], pf)
        assert not np.isin(plans[b]["centres"][:ncenter], r["mask"][b]).any()
    check(r, x, lab, sem, seed, step, B == 5)


def test_golden_slice_and_ball(dev):
    """The reference's generate_occ_point_slice / _ball (recorded draws) replayed through plan=."""
    g = dict(np.load(os.path.join(GOLDEN, "occ.npz")))
    ns, nb = len(g["slice_cloud"]), len(g["ball_cloud"])
    clouds = list(g["slice_cloud"]) + list(g["ball_cloud"])
    x = g["x"][clouds]
    z = np.zeros(x.shape[:2], np.int64)
    plans = [occ_ref.golden_slice_plan(g, i) for i in range(ns)] + [occ_ref.golden_ball_plan(g, i) for i in range(nb)]
    r = run(dev, x, z, z, 5, 3, plans=plans)
    check(r, x, z, z, 5, 3, False)
    for i in range(ns):
        assert np.array_equal(r["mask"][i], g["slice_kept"][i].astype(np.int64))
    for i in range(nb):
        surv = np.unpackbits(g["ball_survivors_packed"][i]).astype(bool)
        m = r["mask"][ns + i]
        assert surv[m].all()
        if surv.sum() == len(m):
            assert np.array_equal(m, np.nonzero(surv)[0])


def test_mixed_batch_drawn_modes(dev):
    B, N = 64, 100
    x, lab, sem = cloud(B, N, 4242)
    r = run(dev, x, lab, sem, 2024, 17, rotate=True)
    check_drawn(r, 2024, 17, N)
    assert len(set(r["plan_i"][:, 0].tolist())) == 4      # every mode occurs among 64 draws
    check(r, x, lab, sem, 2024, 17, True)


@pytest.mark.parametrize("N", [16, 2048])
def test_identical_points_tie_by_index(dev, N):
    K = N // 2
    x = np.full((4, N, 3), 0.25, np.float32)
    z = np.zeros((4, N), np.int64)
    r = run(dev, x, z, z, 8, 0, modes=[0, 1, 2, 3])
    check(r, x, z, z, 8, 0, False)
    # slice: every t is 0, ranks are indices: K-1 .. 2K-2
    assert np.array_equal(r["mask"][2], np.arange(K - 1, 2 * K - 1))
    # ball: each centre cancels the lowest indices (itself only if it is among them)
    nc = int(r["plan_i"][0, 1])
    assert r["mask"][0].min() >= K // nc


@pytest.mark.parametrize("N", [16, 100, 2048])
def test_part_mode_edges(dev, N):
    K = N // 2
    x, lab, _ = cloud(4, N, 31 + N)
    sem = np.full((4, N), 7, np.int64)
    sem[1, N - K:] = 3                 # survivors = K: fallback
    sem[2, N - K - 1:] = 3             # survivors = K + 1: trim
    sem[3, :3] = 3                     # probed at a 7 (below): 3 survivors, fallback
    plans = [dict(occ_ref.draw_plan(6, 1, b, N, occ_ref.PART), probe=0) for b in range(4)]
    plans[3]["probe"] = N - 1
    r = run(dev, x, lab, sem, 6, 1, plans=plans)
    o = check(r, x, lab, sem, 6, 1, False)
    assert [v["branch"] for v in o] == ["part-fallback", "part-fallback", "part-trim", "part-fallback"]
    rnd = run(dev, x, lab, sem, 6, 1, modes=[1] * 4)
    for b in (0, 1, 3):
        assert np.array_equal(r["mask"][b], rnd["mask"][b])
    assert (sem[2][r["mask"][2]] == 3).all()


def test_stateless_and_step_dependent(dev):
    x, lab, sem = cloud(3, 2048, 5)
    a = run(dev, x, lab, sem, 1, 10, rotate=True)
    b = run(dev, x, lab, sem, 1, 10, rotate=True)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    c = run(dev, x, lab, sem, 1, 11, rotate=True)
    assert not np.array_equal(a["mask"], c["mask"])
    d = run(dev, x, lab, sem, 2, 10, rotate=True)
    assert not np.array_equal(a["mask"], d["mask"])


def test_gen_occ_point_names(dev):
    from dataset import gen_occ_point as G
    from ured_hip import occ
    x, lab, sem = cloud(2, 100, 9)
    xt, st = torch.from_numpy(x).to(dev), torch.from_numpy(sem).to(dev)
    for fn, mode, extra in ((G.generate_occ_point_ball, 0, ()), (G.generate_occ_point_random, 1, ()),
                            (G.generate_occ_point_slice, 2, ()), (G.generate_occ_point_part, 3, (st,))):
        pts, mask = fn(xt, *extra, seed=44)
        ref = occ.occlude(xt, st, st, 44, modes=mode)
        assert torch.equal(mask, ref["mask"]) and torch.equal(pts, ref["ori_point_occ"])
        p1, m1 = fn(xt[0], *[e[0] for e in extra], seed=44)
        assert p1.shape == (50, 3) and torch.equal(m1, mask[0]) and torch.equal(p1, pts[0])


def test_argument_checks(dev):
    from ured_hip import occ
    x = torch.zeros(2, 32, 3, device=dev)
    lab = torch.zeros(2, 32, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="MI355X"):
        occ.occlude(x.cpu(), lab.cpu(), lab.cpu(), 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        occ.occlude(x, lab.cpu(), lab, 1)
    with pytest.raises(ValueError, match="N 8"):
        occ.occlude(x[:, :8], lab[:, :8], lab[:, :8], 1)
    with pytest.raises(ValueError, match="int64"):
        occ.occlude(x, lab.int(), lab, 1)
    with pytest.raises(ValueError, match="float32"):
        occ.occlude(x.double(), lab, lab, 1)
    for bad in (4, [0, 7], [-2, 1]):
        with pytest.raises(ValueError, match="outside"):
            occ.occlude(x, lab, lab, 1, modes=bad)
    with pytest.raises(ValueError, match="2 entries"):
        occ.occlude(x, lab, lab, 1, modes=[1, 1, 1])
    a = occ.occlude(x, lab, lab, 1, modes=2)                  # one int == a list == a device tensor
    for m in ([2, 2], torch.tensor([2, 2], device=dev)):
        assert torch.equal(a["mask"], occ.occlude(x, lab, lab, 1, modes=m)["mask"])
    with pytest.raises(ValueError, match="not both"):
        occ.occlude(x, lab, lab, 1, modes=1, plan=(torch.zeros(2, 12, dtype=torch.int32, device=dev),
                                                   torch.zeros(2, 6, device=dev)))
