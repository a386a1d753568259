"""Generate tests/golden/occ.npz FROM THE REFERENCE's dataset/gen_occ_point.py (run where
/root/reference exists; never on the GPU box).

generate_occ_point_slice and generate_occ_point_ball are lifted with `ast` (their module imports
pytorch3d at the top, which is not needed for the functions' own logic) and run with
  * `np.random.*` replaced by stand-ins that replay draws recorded here (the centre index and the
    three direction uniforms of slice; ncenter and the centre indices of ball). The ball trim's
    `np.random.choice(nofoccp, size=surplus, replace=False)` is replayed as "drop nothing", so the
    function returns every point that survived the cancellation: that set is deterministic, the
    reference's trim is a random subset of it;
  * `pytorch3d.ops.knn_points` replaced by a brute-force float32 stand-in: d = ((dx*dx) + (dy*dy))
    + (dz*dz), stable argsort (ties to the lower index), the K nearest.
Recorded (data only): the clouds, the draws, the kept index set of each slice case and the survivor
set of each ball case. The slice cases have float64 gaps in t of at least 1e-4 at both rank
boundaries (K-2|K-1 and N-2|N-1), so a float32 and a float64 evaluation select the same set; a
draw without them is rejected and the next one taken.
    python tests/golden/make_golden_occ.py
"""
import ast
import os
import pickle
import sys
import tempfile
import types

import numpy
import torch

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "387-u-red-unsupervised-3d-shape-retrieval-and-deformation-for-partial-point-clouds_amd"))
from dataset import synthetic  # noqa: E402  (ours: the synthetic cloud generator)

N, K = 2048, 1024
MIN_GAP = 1e-4


class Replay:
    """np.random stand-in: answers the calls of one lifted function from a recorded script."""

    def __init__(self, script):
        self.script = list(script)

    def _next(self, kind):
        k, v = self.script.pop(0)
        assert k == kind, (k, kind)
        return v

    def randint(self, high, size=None):
        v = self._next("randint")
        assert size == 1 and 0 <= v < high
        return numpy.array([v])

    def uniform(self, low=0.0, high=1.0, size=None):
        v = self._next("uniform")
        assert len(v) == size and (v >= low).all() and (v < high).all()
        return numpy.array(v, numpy.float64)

    def choice(self, a, size=None, replace=True):
        v = self._next("choice")
        if size is None:                               # np.random.choice(center_p_choice)
            assert v in list(a)
            return v
        if v is None:                                  # the surplus trim: drop nothing
            return numpy.empty(0, numpy.int64)
        assert len(v) == size and not replace and len(set(v)) == len(v) and max(v) < a
        return numpy.array(v, numpy.int64)


class NumpyWith:
    """`np` of the lifted function: numpy, with .random replaced."""

    def __init__(self, random):
        self.random = random

    def __getattr__(self, name):
        return getattr(numpy, name)


def knn_points_stand_in(p1, p2, K=1, return_sorted=True):
    a = p1[0].numpy().astype(numpy.float32)
    b = p2[0].numpy().astype(numpy.float32)
    idx = numpy.empty((a.shape[0], K), numpy.int64)
    for i in range(a.shape[0]):
        d = b - a[i]
        d = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        assert d.dtype == numpy.float32
        idx[i] = numpy.argsort(d, kind="stable")[:K]
    return types.SimpleNamespace(idx=torch.from_numpy(idx)[None])


def lift(names, ns):
    path = os.path.join(REF, "dataset/gen_occ_point.py")
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)


def run_ref(name, script, *args):
    rnd = Replay(script)
    ns = {"np": NumpyWith(rnd), "os": os, "pickle": pickle, "torch": torch,
          "pytorch3d": types.SimpleNamespace(ops=types.SimpleNamespace(knn_points=knn_points_stand_in))}
    lift(["generate_occ_point_slice", "generate_occ_point_ball", "generate_occ_point_random"], ns)
    pts, mask = ns[name](*args)
    assert not rnd.script, "unused recorded draws"
    assert (pts == args[0][mask]).all()
    return numpy.asarray(mask)


def main():
    x = synthetic.make_batch(3, N, 8, parts=4, seed=2024)["x"].astype(numpy.float32)
    rng = numpy.random.Generator(numpy.random.PCG64(7))
    out = {"x": x}
    # ---- slice: clouds 0 and 1 ----
    sc, su, sd, sk = [], [], [], []
    for cloud in (0, 1):
        while True:
            centre = int(rng.integers(0, N))
            u = rng.uniform(1e-3, 1.0, size=3)
            direction = u / numpy.linalg.norm(u)
            t = numpy.sort(numpy.abs((x[cloud].astype(numpy.float64) - x[cloud, centre]) @ direction))
            if t[K - 1] - t[K - 2] >= MIN_GAP and t[N - 1] - t[N - 2] >= MIN_GAP:
                break
        mask = run_ref("generate_occ_point_slice", [("randint", centre), ("uniform", u)], x[cloud])
        assert mask.shape == (K,) and len(set(mask.tolist())) == K
        sc.append(centre), su.append(u), sd.append(direction), sk.append(numpy.sort(mask))
    out.update(slice_cloud=numpy.array([0, 1]), slice_centre=numpy.array(sc), slice_uniform=numpy.array(su),
               slice_direction=numpy.array(sd), slice_kept=numpy.array(sk, numpy.int16))
    # ---- ball: cloud 2 with one centre (no surplus) and with four (overlapping balls: a surplus) ----
    bn, bc, bs = [], [], []
    for ncenter in (1, 4):
        centres = [int(v) for v in rng.choice(N, size=ncenter, replace=False)]
        with tempfile.TemporaryDirectory() as tmp:
            mask = run_ref("generate_occ_point_ball", [("choice", ncenter), ("choice", centres), ("choice", None)][:2 + (ncenter > 1)],
                           x[2], 0, tmp)
        surv = numpy.zeros(N, numpy.uint8)
        surv[mask] = 1
        assert surv.sum() == len(mask) >= K and (ncenter > 1 or surv.sum() == K)
        bn.append(ncenter), bc.append(centres + [-1] * (8 - ncenter)), bs.append(numpy.packbits(surv))
    out.update(ball_cloud=numpy.array([2, 2]), ball_ncenter=numpy.array(bn), ball_centres=numpy.array(bc),
               ball_survivors_packed=numpy.array(bs))
    dst = os.path.join(HERE, "occ.npz")
    numpy.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; ball survivors", [int(numpy.unpackbits(b).sum()) for b in bs])


if __name__ == "__main__":
    main()
