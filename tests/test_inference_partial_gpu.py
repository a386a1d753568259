"""Partial (occluded) targets through the loaders and the inference path: engine/test.py
infer_partial, GraphedInfer on the partial sub-batch, the "partial" loader key, and the training
step ignoring the new batch keys."""
import numpy as np
import pytest
import torch

from oracle import ured_ref

pytestmark = pytest.mark.gpu

CFG = {"source_latent_dim": 64, "target_latent_dim": 64, "sem_latent_dim": 16, "MAX_NUM_PARTS": 16,
       "alpha": 0.1, "device": "cuda", "optimizer": "adam", "learning_rate": 1e-3, "weight_decay": 5e-4,
       "lr_stepsize": 3, "lr_decay": 0.5, "momentum": 0.9}
TRAIN = dict(CFG, use_chamfer_loss=30.0, use_chamfer_part_loss=1.0, use_symmetry_loss=30.0, use_contrast_loss=0.5,
             use_param_loss=0.0, init_p_m_loss=-1, use_residuals_reg=3.0, use_recon=30.0, batch_size=2,
             num_points=128, parts=3, iters_per_epoch=2)
NS = 300


@pytest.fixture(scope="module")
def world(dev):
    from dataset import synthetic
    from train_utils.load_sources import SourceDB
    from engine.train import get_models
    from engine.test import encode_sources
    dbn = synthetic.make_source_db(NS, seed=51)
    db = SourceDB(dbn["src_points"], dbn["src_mats"], dbn["src_default_param"], dbn["src_sem"], dev)
    models, _, _ = get_models(CFG, dev)
    for name, sd in ured_ref.make_params(CFG, seed=5).items():
        models[name].load_state_dict({k: (v + 0.05 if "running_var" in k else v) for k, v in sd.items()}, strict=True)
    return db, models, encode_sources(models, db)


def partial_batch(dev, seed, rotate=True, parts=(4, 2, 7)):
    from dataset import synthetic
    from engine.train import add_partial, batch_to_device
    bt = synthetic.make_batch(len(parts), 256, NS, parts=list(parts), seed=seed)
    return add_partial(batch_to_device(bt, dev), dict(CFG, random_rot=rotate), seed=7, epoch=1, it=seed)


def test_infer_partial_is_infer_on_the_gathered_sub_batch(dev, world):
    from engine.test import infer, infer_partial
    db, models, codes = world
    b = partial_batch(dev, 60)
    m = b["point_occ_mask"]
    assert m.shape == (3, 128) and torch.equal(b["ori_point_occ"], b["x"].gather(1, m.unsqueeze(-1).expand(-1, -1, 3)))
    sub = {"x": b["point_occ"], "labels": b["labels"].gather(1, m), "tgt_sem": b["tgt_sem"].gather(1, m)}
    ref = infer(models, db, sub, CFG, codes)
    got = infer_partial(models, db, b, CFG, codes)
    for k in ("retrieved", "params", "out", "cd", "mask"):
        assert torch.equal(got[k], ref[k]), k
    # cd_full: the inverse transform and the chamfer composed in torch (float64)
    out = got["out"].double() @ b["occ_rot"].double() + b["occ_mean"].double().unsqueeze(1)
    x = b["x"].double()
    for i in range(3):
        d = torch.cdist(out[i], x[i]) ** 2
        cd = d.min(1).values.mean() + d.min(0).values.mean()
        assert abs(got["cd_full"][i].item() - cd.item()) <= 1e-5 * abs(cd.item()), (i, got["cd_full"][i].item(), cd.item())
    # that transform is the inverse of the generator's: it takes point_occ back to ori_point_occ (fp32
    # roundings of point_occ, occ_rot and occ_mean: a few 1e-7 for coordinates in [-1, 1]); the
    # transposed rotation does not (|(R - R^T) p| ~ 2 sin(angle) |p|, angles up to 10 degrees)
    rot, mean, ori = b["occ_rot"].double(), b["occ_mean"].double().unsqueeze(1), b["ori_point_occ"].double()
    assert rot.float().sub(torch.eye(3, device=dev)).abs().max() > 1e-3
    assert (b["point_occ"].double() @ rot + mean - ori).abs().max() <= 2e-6
    assert (b["point_occ"].double() @ rot.transpose(1, 2) + mean - ori).abs().max() > 1e-4


def test_removed_part_is_an_empty_slot(dev, world):
    """Part occlusion of a part with a semantic class of its own removes the whole part."""
    from dataset import synthetic
    from engine.train import batch_to_device
    from engine.test import infer_partial
    from ured_hip import occ
    import occ_ref
    db, models, codes = world
    parts = [4, 5]
    bt = synthetic.make_batch(2, 256, NS, parts=parts, seed=61)
    bt["tgt_sem"] = bt["labels"].copy()                      # one semantic class per part
    b = batch_to_device(bt, dev)
    removed = [2, 0]
    plans = []
    for i in range(2):
        p = occ_ref.draw_plan(3, 0, i, 256, occ_ref.PART)
        p["probe"] = int(np.nonzero(bt["labels"][i] == removed[i])[0][0])
        plans.append(occ_ref.plan_arrays(p))
    plan = tuple(torch.from_numpy(np.stack(a)).to(dev) for a in zip(*plans))
    r = occ.occlude(b["x"], b["labels"], b["tgt_sem"], 3, 0, plan=plan)
    for i in range(2):
        assert removed[i] not in r["labels_occ"][i].tolist()
        assert set(r["labels_occ"][i].tolist()) == set(range(parts[i])) - {removed[i]}
    b.update(point_occ=r["point_occ"], labels_occ=r["labels_occ"], tgt_sem_occ=r["sem_occ"],
             occ_mean=r["occ_mean"], occ_rot=r["occ_rot"])
    got = infer_partial(models, db, b, CFG, codes)
    for i in range(2):
        k = parts[i] - 1                                     # the surviving parts fill slots [0, k)
        assert got["mask"][i].tolist() == [1.0] * k + [0.0] * (16 - k)
        assert (got["retrieved"][i, :k] >= 0).all() and (got["retrieved"][i, k:] == -1).all()
    assert bool(torch.isfinite(got["cd_full"]).all())


def test_graphed_infer_accepts_the_partial_sub_batch(dev, world):
    from engine.test import GraphedInfer, infer, infer_partial, partial_sub_batch
    db, models, codes = world
    gi = GraphedInfer(models, db, CFG, codes)
    for i in range(3):                                       # eager + capture, then two replays
        b = partial_batch(dev, 70 + i)
        got = infer_partial(models, db, b, CFG, codes, run=gi)
        ref = infer(models, db, partial_sub_batch(b), CFG, codes)
        for k in ("retrieved", "params", "out", "cd", "re_score", "sim_top2_gap"):
            assert torch.equal(got[k], ref[k]), (i, k)
        assert torch.equal(got["cd_full"], infer_partial(models, db, b, CFG, codes)["cd_full"])
    assert len(gi.graphs) == 1


@pytest.mark.parametrize("rot", [False, True])
def test_partial_loader_keys(dev, rot):
    from engine.config import PARTIAL_KEYS
    from engine.train import SyntheticLoader
    cfg = dict(TRAIN, partial=True, random_rot=rot)
    plain = list(SyntheticLoader(dict(TRAIN), 24, dev, seed=2))
    loader = SyntheticLoader(cfg, 24, dev, seed=2)
    first = list(loader)
    assert len(first) == 2
    shapes = {"point_occ": ((2, 64, 3), torch.float32), "point_occ_mask": ((2, 64), torch.int64),
              "ori_point_occ": ((2, 64, 3), torch.float32), "labels_occ": ((2, 64), torch.int64),
              "tgt_sem_occ": ((2, 64), torch.int64), "occ_mean": ((2, 3), torch.float32),
              "occ_rot": ((2, 3, 3), torch.float32)}
    assert set(shapes) == set(PARTIAL_KEYS)
    for b, p in zip(first, plain):
        assert not any(k in p for k in PARTIAL_KEYS)
        for k, (shape, dtype) in shapes.items():
            assert tuple(b[k].shape) == shape and b[k].dtype == dtype and b[k].is_cuda, k
        assert torch.equal(b["x"], p["x"]) and torch.equal(b["labels"], p["labels"])
        m = b["point_occ_mask"]
        assert torch.equal(b["labels_occ"], b["labels"].gather(1, m)) and torch.equal(b["tgt_sem_occ"], b["tgt_sem"].gather(1, m))
        eye = torch.eye(3, device=dev).expand(2, 3, 3)
        assert torch.equal(b["occ_rot"], eye) != rot
    # (seed, epoch, iteration): iterations differ, the next epoch differs, a new loader repeats
    assert not torch.equal(first[0]["point_occ_mask"], first[1]["point_occ_mask"])
    second = list(loader)
    assert not torch.equal(first[0]["point_occ_mask"], second[0]["point_occ_mask"])
    again = list(SyntheticLoader(cfg, 24, dev, seed=2))
    assert all(torch.equal(a[k], f[k]) for a, f in zip(again, first) for k in PARTIAL_KEYS)


def test_pseudo_label_loader_partial_keys(dev, tmp_path):
    """PseudoLabelLoader with "partial": each batch's partial view is occlude() of that batch at
    (loader seed, epoch << 32 | iteration), over two epochs of the shuffled target set."""
    import json
    import os
    from conftest import PKG_DIR
    from engine.config import PARTIAL_KEYS
    from engine.train import PseudoLabelLoader
    from train_utils.load_sources import load_sources
    from ured_hip import occ
    with open(os.path.join(PKG_DIR, "config", "config_train_test.json")) as f:
        cfg = json.load(f)
    cfg.update(source_latent_dim=64, target_latent_dim=64, part_latent_dim=64, sem_latent_dim=16, batch_size=2,
               num_points=256, num_source=48, num_targets=4, parts=3, log_path=str(tmp_path), device="cuda", cl_k=8,
               partial=True, random_rot=True)
    db, dist_src = load_sources(cfg, dev)
    ld = PseudoLabelLoader(cfg, db, dev, dist_src, seed=3)
    names = {"point_occ": "point_occ", "point_occ_mask": "mask", "ori_point_occ": "ori_point_occ",
             "labels_occ": "labels_occ", "tgt_sem_occ": "sem_occ", "occ_mean": "occ_mean", "occ_rot": "occ_rot"}
    assert set(names) == set(PARTIAL_KEYS)
    seen = []
    for epoch in range(2):
        batches = list(ld)
        assert len(batches) == 2
        for it, b in enumerate(batches):
            ref = occ.occlude(b["x"], b["labels"], b["tgt_sem"], 3, (epoch << 32) | it, rotate=True)
            for k, r in names.items():
                assert torch.equal(b[k], ref[r]), (epoch, it, k)
            other = occ.occlude(b["x"], b["labels"], b["tgt_sem"], 3, ((epoch + 1) << 32) | it, rotate=True)
            assert not torch.equal(b["point_occ_mask"], other["mask"])
            seen.append(b["point_occ_mask"].clone())
    assert seen[0].shape == (2, 128) and seen[0].dtype == torch.int64


def test_train_step_ignores_the_partial_keys(dev):
    from dataset import synthetic
    from train_utils.load_sources import SourceDB
    from engine.train import SyntheticLoader, TrainStep
    dbn = synthetic.make_source_db(24, seed=3)
    db = SourceDB(dbn["src_points"], dbn["src_mats"], dbn["src_default_param"], dbn["src_sem"], dev)
    losses = []
    for partial in (False, True):
        cfg = dict(TRAIN, partial=partial, random_rot=True)
        ts = TrainStep(cfg, db, dev)
        for name, sd in ured_ref.make_params(cfg, seed=7).items():
            ts.models[name].load_state_dict(sd, strict=True)
        run = []
        for b in SyntheticLoader(cfg, 24, dev, seed=9):
            assert ("point_occ" in b) == partial
            T = ts.step(b)
            run.append({k: torch.as_tensor(v).detach().cpu().clone() for k, v in T.items()
                        if torch.is_tensor(v) or isinstance(v, float)})
        losses.append(run)
    assert len(losses[0]) == 2 and "all_loss" in losses[0][0]
    for a, b in zip(*losses):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_graphed_step_ignores_the_partial_keys(dev):
    """GraphedStep drops the partial keys before keying / cloning / refreshing its static batch:
    captured and replayed steps on a "partial" loader equal eager steps without it, bitwise."""
    from dataset import synthetic
    from train_utils.load_sources import SourceDB
    from engine.graph import GraphedStep
    from engine.train import SyntheticLoader, TrainStep
    dbn = synthetic.make_source_db(24, seed=3)
    db = SourceDB(dbn["src_points"], dbn["src_mats"], dbn["src_default_param"], dbn["src_sem"], dev)
    steps = []
    for partial in (False, True):
        cfg = dict(TRAIN, partial=partial, cuda_graph=True, iters_per_epoch=1)
        ts = TrainStep(cfg, db, dev)
        for name, sd in ured_ref.make_params(cfg, seed=7).items():
            ts.models[name].load_state_dict(sd, strict=True)
        steps.append((GraphedStep(ts) if partial else ts, SyntheticLoader(cfg, 24, dev, seed=9)))
    (eager, plain), (graphed, part) = steps
    for _ in range(3):                                       # eager + capture, then replays
        (a,), (b,) = list(plain), list(part)
        assert "point_occ" in b and "point_occ" not in a
        la, lb = eager.step(a)["all_loss"].detach().clone(), graphed.step(b)["all_loss"].detach().clone()
        assert torch.equal(la, lb)
