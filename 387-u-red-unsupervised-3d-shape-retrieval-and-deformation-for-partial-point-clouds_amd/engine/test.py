"""Retrieval + deformation inference (the working form of the reference's inference path).

The reference's engine/test.py no longer runs against its own modules; the
working path is engine/vis.py:118-256, restated here batched and without host syncs:
  1. encode the whole source-part DB with src_encoder_all in eval mode (chunks of 512 parts,
     vis.py:126-145) -> L2-normalised codes [NS, C]
  2. encode the targets (eval), pool per-part features (vis.py:175-195), L2-normalise
  3. cosine similarity target parts x sources, argmax -> retrieved source per part (vis.py:197-205)
  4. DeformNet on (target code, normalised retrieved codes) -> params; get_shape with the
     retrieved sources' A matrices and no default param (vis.py:243-252)
  5. chamfer of the deformed shape (all 16x1024 points, the unmasked branch vis.py:256 lands in)
  6. (optional) the residual-net score max_points sum|r| (vis.py:221-231), NDCG@40 of the
     retrieval scores against the pseudo-label rows (cal_retrieval_score, vis.py:207), and the
     retrieved meshes deformed with the target parts' boxes as default (vis.py:278-296)
  7. (optional, cfg["partial"]) the same from a partial view of each target, generated on the
     device (ured_hip.occ; the reference dataset's points_occ), with the chamfer also taken against
     the complete target in its own frame: infer_partial
    python engine/test.py [config.json]       (default config/config_vis_test.json, the reference's
                                              inference schema read by engine/vis.py:29; its
                                              init_dm / init_re checkpoints are loaded as the
                                              reference does, get_models)
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(_HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(_HERE))

from dataset import synthetic  # noqa: E402
from dataset.dataset_utils import cal_retrieval_score, deform_vertices, get_shape  # noqa: E402
from engine.train import add_partial, batch_to_device, get_models, get_part  # noqa: E402
from loss.chamfer_loss import compute_cm_loss  # noqa: E402
from train_utils.load_sources import load_sources  # noqa: E402
from ured_hip.ops import refresh_static  # noqa: E402


@torch.no_grad()
def encode_sources(models, db, chunk=512):
    enc = models["src_encoder_all"]
    emb = models["embedding_layer"]
    codes = []
    for s in range(0, db.num_sources, chunk):
        pts = db.points[s:s + chunk].unsqueeze(1)                  # [n, 1, 1024, 3]
        sem = emb(db.sem[s:s + chunk]).unsqueeze(1)                # [n, 1, S]
        c, _ = enc.forward_pointmajor(pts, sem)
        codes.append(c)
    return F.normalize(torch.cat(codes), dim=-1, p=2)


@torch.no_grad()
def infer(models, db, batch, cfg, src_codes=None, relevance=None, meshes=None):
    """-> dict(retrieved [B,P] (-1 for empty slots), sim_top2_gap [B,P], params [B,P,6],
    out [B,P*1024,3], cd [B] (chamfer_distance2 of out vs x), re_score [B]) plus, with
    `relevance` ([B,P,NS] pseudo-label cd_m rows of the target parts), ndcg [B,P] (NaN for empty
    slots), and with `meshes` ({"vmats","voff"} device tensors of the source DB), the deformed
    retrieved meshes (vertices [R,3], vertex offsets [B*P+1])."""
    for m in models.values():
        m.eval()
    if src_codes is None:
        src_codes = encode_sources(models, db)
    x = batch["x"]
    B, N, _ = x.shape
    P = cfg["MAX_NUM_PARTS"]
    tcode, pp = models["target_encoder_full"].forward_pointmajor(x, models["embedding_layer"](batch["tgt_sem"]))
    part_f, _, re_in, mask, _, param_def = get_part(cfg, pp.view(B, N, -1), batch["labels"], x)
    part_n = F.normalize(part_f, dim=-1, p=2)
    sim = part_n @ src_codes.t()                                      # [B, P, NS]
    top2 = sim.topk(2, dim=-1).values
    retrieved = sim.argmax(dim=-1)
    retrieved = torch.where(mask > 0, retrieved, torch.full_like(retrieved, -1))
    idx = torch.where(retrieved < 0, retrieved + db.num_sources, retrieved)
    params = models["param_decoder_full"](tcode, src_codes[idx], None)
    out = get_shape(db.mats[idx], params, None, cfg["alpha"]).reshape(B, -1, 3)
    cd = compute_cm_loss(out, x, mask, batch_reduction=None)          # unmasked branch, like vis.py:256
    res = models["re_residual_net_full"].forward_split(re_in.pp_sorted, re_in.part_mean, gidx=re_in.gid,
                                                        off=re_in.off).view(B, N, 3)
    r = {"retrieved": retrieved, "sim_top2_gap": top2[..., 0] - top2[..., 1], "params": params,
         "out": out, "cd": cd, "mask": mask, "re_score": res.abs().sum(-1).amax(-1)}
    if relevance is not None:
        nd = cal_retrieval_score(sim.reshape(B * P, -1), relevance.reshape(B * P, -1)).view(B, P)
        r["ndcg"] = torch.where(mask > 0, nd, torch.full_like(nd, float("nan")))
    if meshes is not None:
        r["vertices"], r["vertex_off"] = deform_vertices(meshes["vmats"], meshes["voff"], idx, params,
                                                         param_def, cfg["alpha"])
    return r


def partial_sub_batch(batch):
    """The partial view of a loader batch (cfg["partial"]) as an infer() / GraphedInfer batch."""
    return {"x": batch["point_occ"], "labels": batch["labels_occ"], "tgt_sem": batch["tgt_sem_occ"]}


@torch.no_grad()
def infer_partial(models, db, batch, cfg, src_codes=None, run=None, **kw):
    """Retrieval + deformation from the partial view of `batch` (the keys a cfg["partial"] loader
    adds, engine/train.py add_partial): infer() on (point_occ, labels_occ, tgt_sem_occ) — the
    occluded, centred (and rotated) cloud is all the networks see; a part without a surviving point
    is an empty slot (mask 0, retrieved -1) — and its dict plus
      cd_full [B]: the deformed output mapped back to the full shape's frame (out @ occ_rot +
                   occ_mean, the inverse of point_occ = (occ_rot @ (ori - mean)^T)^T) scored with the
                   same unmasked chamfer against the complete target batch["x"].
    `run` (optional): a GraphedInfer to replay instead of the eager infer(); its outputs are the
    captured tensors."""
    sub = partial_sub_batch(batch)
    r = dict(run(sub, **kw) if run is not None else infer(models, db, sub, cfg, src_codes, **kw))
    full = torch.baddbmm(batch["occ_mean"].unsqueeze(1), r["out"], batch["occ_rot"])
    r["cd_full"] = compute_cm_loss(full, batch["x"], r["mask"], batch_reduction=None)
    return r


class GraphedInfer:
    """infer() as one HIP graph per batch shape (torch.cuda.CUDAGraph = hipGraph). A 16-target
    batch is ~3 ms of host launches (a few hundred small kernels) for well under 1 ms of GPU
    work; infer() has no host sync, so it is captured once per shape key and replayed: inputs
    are copied into the captured batch, the outputs are the captured tensors (overwritten by the
    next call; clone what must outlive it). Same kernels and arithmetic as the eager call: a
    replay is bit-identical to infer() on the same models, codes and batch. The optional extras
    run eagerly (meshes have a data-dependent vertex count)."""

    def __init__(self, models, db, cfg, src_codes, max_graphs=4):
        self.models, self.db, self.cfg, self.codes = models, db, cfg, src_codes
        self.max_graphs = max_graphs
        self.graphs = {}

    INPUTS = ("x", "labels", "tgt_sem")           # what infer() reads from a batch

    @classmethod
    def key(cls, batch):
        return tuple((k, tuple(batch[k].shape), batch[k].dtype) for k in cls.INPUTS)

    def __call__(self, batch, relevance=None, meshes=None):
        if relevance is not None or meshes is not None:
            return infer(self.models, self.db, batch, self.cfg, self.codes, relevance, meshes)
        k = self.key(batch)
        ent = self.graphs.get(k)
        if ent is None:
            # eager run on a side stream first (initialises library handles / workspaces for the
            # capture), then capture on a clone of the batch
            main = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                r = infer(self.models, self.db, batch, self.cfg, self.codes)
            main.wait_stream(side)
            static = {n: batch[n].clone() for n in self.INPUTS}
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = infer(self.models, self.db, static, self.cfg, self.codes)
            if len(self.graphs) >= self.max_graphs:
                self.graphs.pop(next(iter(self.graphs)))
            self.graphs[k] = (static, g, out)
            return r
        static, g, out = ent
        refresh_static(static, {n: batch[n] for n in self.INPUTS})    # one batched copy launch
        g.replay()
        return out


def main(cfg):
    for key in ("dm_model_path", "re_model_path"):
        flag = "init_dm" if key == "dm_model_path" else "init_re"
        if cfg.get(flag) and not os.path.exists(cfg[key]):
            raise FileNotFoundError(f"{flag} is set but {cfg[key]} does not exist (train first: "
                                    f"python engine/train.py writes {cfg.get('log_path', '.')}/checkpoint_*.pth)")
    device = cfg["device"]
    db, _ = load_sources(dict(cfg, compute_connectivity=False), device)
    models, _, _ = get_models(cfg, device)
    codes = encode_sources(models, db)
    for i in range(int(cfg.get("iters_per_epoch", 2))):
        b = synthetic.make_batch(cfg["batch_size"], cfg.get("num_points", 2048), db.num_sources,
                                 max_parts=cfg["MAX_NUM_PARTS"], parts=cfg.get("parts", 4), seed=10_000 + i)
        bd = batch_to_device(b, device)
        if cfg.get("partial"):
            r = infer_partial(models, db, add_partial(bd, cfg, cfg.get("seed", 0), 0, i), cfg, codes)
            print(i, "cd", r["cd"].mean().item(), "cd_full", r["cd_full"].mean().item(),
                  "retrieved[0]", r["retrieved"][0].tolist())
            continue
        r = infer(models, db, bd, cfg, codes)
        print(i, "cd", r["cd"].mean().item(), "retrieved[0]", r["retrieved"][0].tolist())


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(_HERE), "config", "config_vis_test.json")
    main(json.load(open(path)))
