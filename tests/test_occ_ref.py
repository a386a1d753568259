"""CPU checks of the partial-cloud generator's oracle (tests/occ_ref.py) against the reference's
own gen_occ_point.py (tests/golden/occ.npz, made by tests/golden/make_golden_occ.py), its
invariants, the plan draw's frequencies, and ured_occlude's argument validation (no GPU)."""
import os

import numpy as np
import pytest

import occ_ref
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "occ.npz")))


def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32_10."""
    got = occ_ref.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    got = occ_ref.philox4x32_10((f, f, f, f), (f, f))
    assert [int(v) for v in got] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_slice_matches_reference(golden):
    g = golden
    for i in range(len(g["slice_cloud"])):
        x = g["x"][g["slice_cloud"][i]]
        # the recorded direction is the reference's own normalisation of the recorded uniforms
        u = g["slice_uniform"][i]
        np.testing.assert_allclose(g["slice_direction"][i], u / np.linalg.norm(u), rtol=1e-15)
        kept, branch = occ_ref.select(x, np.zeros(len(x), np.int64), occ_ref.golden_slice_plan(g, i), 1, 0, 0)
        assert branch == "slice"
        assert np.array_equal(kept, g["slice_kept"][i].astype(np.int64))


def test_ball_matches_reference(golden):
    g = golden
    for i in range(len(g["ball_cloud"])):
        x = g["x"][g["ball_cloud"][i]]
        K = len(x) // 2
        plan = occ_ref.golden_ball_plan(g, i)
        surv = np.unpackbits(g["ball_survivors_packed"][i]).astype(bool)
        assert np.array_equal(occ_ref.ball_survivors(x, plan), surv)
        kept, _ = occ_ref.select(x, np.zeros(len(x), np.int64), plan, 5, 3, 0)
        assert len(kept) == K and surv[kept].all()
        if surv.sum() == K:                       # one centre: nothing to trim, the sets are equal
            assert np.array_equal(kept, np.nonzero(surv)[0])
        else:
            assert plan["ncenter"] > 1


def _cloud(N, seed, nsem=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    return x, rng.integers(0, 5, size=N), rng.integers(0, nsem, size=N)


@pytest.mark.parametrize("N", [16, 100, 2048])
def test_invariants(N):
    K = N // 2
    x, labels, sem = _cloud(N, N)
    for mode in range(4):
        for nc in ((1, 2, 4, 8) if mode == occ_ref.BALL else (None,)):
            plan = occ_ref.draw_plan(11, 2, 3, N, mode)
            assert len(set(plan["centres"].tolist())) == 8
            if nc:
                plan["ncenter"] = nc
            r = occ_ref.occlude_one(x, labels, sem, 11, 2, 3, plan=plan, rotate=True)
            m = r["mask"]
            assert m.shape == (K,) and (np.diff(m) > 0).all() and m[0] >= 0 and m[-1] < N
            assert np.array_equal(r["ori_point_occ"], x[m]) and np.array_equal(r["sem_occ"], sem[m])
            if mode == occ_ref.BALL:
                assert not np.isin(plan["centres"][:nc], m).any()          # each centre cancels itself
            if mode == occ_ref.SLICE:
                d = x - x[plan["slice_centre"]]
                t = np.abs(d.astype(np.float64) @ plan["direction"].astype(np.float64))
                order = np.argsort(t, kind="stable")
                # far half, less the farthest point (ties aside: none in these clouds at the boundaries)
                assert np.array_equal(np.sort(order[K - 1:2 * K - 1]), m)
            np.testing.assert_allclose(r["point_occ"] @ r["occ_rot"] + r["occ_mean"], x[m], atol=1e-12)
            np.testing.assert_allclose(r["occ_rot"] @ r["occ_rot"].T, np.eye(3), atol=1e-14)


@pytest.mark.parametrize("N", [16, 100, 2048])
def test_part_mode_branches(N):
    K = N // 2
    x, labels, _ = _cloud(N, 100 + N)
    plan = occ_ref.draw_plan(4, 0, 0, N, occ_ref.PART)
    plan["probe"] = 0
    for survivors, branch in ((0, "part-fallback"), (K, "part-fallback"), (K + 1, "part-trim")):
        sem = np.full(N, 7, np.int64)
        sem[N - survivors:] = 3                    # the probe (point 0) has semantic 7
        m, got = occ_ref.select(x, sem, plan, 4, 0, 0)
        assert got == branch
        ref, _ = occ_ref.select(x, sem, dict(plan, mode=occ_ref.RANDOM), 4, 0, 0)
        if branch == "part-fallback":
            assert np.array_equal(m, ref)
        else:
            assert (sem[m] == 3).all() and len(m) == K


def test_plan_frequencies():
    n = 4000
    modes, ncs = np.zeros(4), np.zeros(4)
    for s in range(n):
        p = occ_ref.draw_plan(123, s // 100, s % 100, 16)
        modes[p["mode"]] += 1
        ncs[{1: 0, 2: 1, 4: 2, 8: 3}[p["ncenter"]]] += 1
    for cnt, p in list(zip(modes, (0.3, 0.3, 0.3, 0.1))) + list(zip(ncs, (0.25,) * 4)):
        assert abs(cnt - n * p) <= 5 * np.sqrt(n * p * (1 - p)), (modes, ncs)


def test_occlude_rejects_bad_n_without_gpu(built):
    """Argument validation happens before any device work (as test_abi.py's)."""
    from ured_hip import _lib
    import ured_hip.occ  # noqa: F401  (binds ured_occlude)
    for N in (8, 5000):
        with pytest.raises(_lib.UredError, match=f"N {N}"):
            _lib.call("ured_occlude", None, None, None, 1, N, 1, 0, None, -1, None, None, 0, *([None] * 10))
    # an empty batch is valid and launches nothing; it also leaves the thread's last error cleared
    _lib.call("ured_occlude", None, None, None, 0, 2048, 1, 0, None, -1, None, None, 0, *([None] * 10))
    assert _lib.lib().ured_last_error() == b""


def test_wrapper_rejects_cpu_tensors(built):
    import torch
    from ured_hip import occ
    x = torch.zeros(1, 32, 3)
    lab = torch.zeros(1, 32, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X"):
        occ.occlude(x, lab, lab, seed=1)


def test_partial_loader_needs_a_gpu(built):
    """cfg["partial"] on a CPU device raises instead of falling back."""
    from engine.train import SyntheticLoader
    cfg = {"MAX_NUM_PARTS": 16, "batch_size": 2, "num_points": 64, "parts": 3, "iters_per_epoch": 1, "partial": True}
    assert "point_occ" not in next(iter(SyntheticLoader(dict(cfg, partial=False), 24, "cpu", seed=2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(SyntheticLoader(cfg, 24, "cpu", seed=2)))
