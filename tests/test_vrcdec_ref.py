"""tests/vrcdec_ref.py (the float64 restatement the GPU tests of VRCNet's decoder compare against) pinned to the
reference's own EF_expansion, Folding and MSAP_SKN_decoder through tests/golden/vrcdec.npz, the margin rule of
the value-dependent decisions, and the CPU-side checks of the new modules: the grid, state_dict keys and shapes,
and argument validation before any device work."""
import os

import numpy as np
import pytest
import torch

import vrc_ref as R
import vrcdec_ref as D
from conftest import GOLDEN

REL = 1e-9
RATIO_REL = 0.1
NAMES = ("ef", "fold", "dec_fold", "dec_ef")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "vrcdec.npz"))


@pytest.fixture(scope="module")
def runs():
    return {(n, d): D.run_fixture(n, d) for n in NAMES for d in (torch.float64, torch.float32)}


def _close(what, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{what:60s} err {err:.3e} max {scale:.3e}")
    assert err <= REL * scale, f"{what}: {err:.3e} > {REL} x {scale:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference(gold, runs, name):
    assert {k: int(gold[f"seed/{k}"]) for k in D.GOLDEN_SEEDS} == D.GOLDEN_SEEDS
    res = runs[name, torch.float64]
    n_out = 4 if name.startswith("dec") else 1
    for i in range(n_out):
        _close(f"{name} out{i}", res["outs"][i], gold[f"{name}/out{i}"])
    keys = [k[len(name) + 3:] for k in gold.files if k.startswith(f"{name}/g/")]
    assert set(keys) == set(res["grads"]) - res["none"], set(keys) ^ (set(res["grads"]) - res["none"])
    for k in keys:
        _close(f"{name} grad {k}", R.grad_sub(res["grads"][k]), gold[f"{name}/g/{k}"])
    if name.startswith("dec"):                       # conv_s1..3 feed the selection only: no gradient in the reference either
        assert res["none"] == {f"conv_s{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")}


def test_decisions_match_the_reference(gold, runs):
    assert np.array_equal(runs["ef", torch.float64]["dec"].idx["ef.knn"].numpy(), gold["ef/knn"])
    for name in D.DECS:
        dec = runs[name, torch.float64]["dec"]
        assert np.array_equal(dec.idx["fps"].numpy(), gold[f"{name}/fps"])
        assert np.array_equal(dec.idx["topk"].numpy(), gold[f"{name}/topk"])
        for lv in (1, 2, 3):
            assert np.array_equal(dec.enc.idx[f"fps{lv}"].numpy(), gold[f"{name}/enc_fps{lv}"])
        tags = [k[len(name) + 5:] for k in gold.files if k.startswith(f"{name}/knn/")]
        assert tags == (["exp1", "exp2"] if name == "dec_ef" else [])
        for tag in tags:
            assert np.array_equal(dec.idx[tag + ".knn"].numpy(), gold[f"{name}/knn/{tag}"])


@pytest.mark.parametrize("name", ["ef", "dec_fold", "dec_ef"])
def test_value_dependent_decisions_keep_their_margin(gold, runs, name):
    """Every rank gap of the feature-space kNN, every FPS winner against its runner-up and every gap among the
    first num_coarse + 1 score ranks, in float64, is at least MARGIN_MULT times the forward tolerance of the
    deciding quantity; the encoder's geometry keeps GEO_MARGIN; float32 makes the same decisions."""
    r64, r32 = runs[name, torch.float64], runs[name, torch.float32]
    ratios = D.decision_ratios(r64, r32)
    print(name, {k: round(v, 3) for k, v in ratios.items()})
    want = {"ef": {"ef.knn"}, "dec_fold": {"fps", "topk"}, "dec_ef": {"exp1.knn", "exp2.knn", "fps", "topk"}}[name]
    assert set(ratios) == want
    worst = min(ratios.values())
    # the recorded ratio: err(ref32, ref64) in its denominator depends on the CPU's float32 summation order
    # (1.4 % between two machines for dec_fold), so it is compared to RATIO_REL; the rule below is not loosened
    assert abs(worst - D.GOLDEN_RATIOS[name]) <= RATIO_REL * worst, (worst, D.GOLDEN_RATIOS[name])
    assert abs(float(gold[f"ratio/{name}"]) - D.GOLDEN_RATIOS[name]) <= 1e-9 * worst
    if name != "ef":
        for dtype, res in ((torch.float64, r64), (torch.float32, r32)):
            enc = res["dec"].enc
            names = D.geo_names(enc)
            assert len(names) == 4 * len(D.DECS[name]["knn_list"]) + 3 + 3 + 3
            for k in names:
                assert enc.margin[k] >= R.GEO_MARGIN * (1 if dtype == torch.float64 else 0.99), (k, enc.margin[k])
        for k, v in r64["dec"].enc.idx.items():
            if not k.startswith(("slot", "win")):
                assert torch.equal(v, r32["dec"].enc.idx[k]), k
    for k, v in r64["dec"].idx.items():
        if not k.endswith(".slot"):
            assert torch.equal(v, r32["dec"].idx[k]), k
    assert worst >= D.MARGIN_MULT, f"{name}: the smallest gap is {worst:.3f} x the tolerance, the rule asks for {D.MARGIN_MULT}"


@pytest.mark.parametrize("r", [1, 2, 3, 4, 6])
def test_folding_grid(gold, r):
    from chamfer3D.model_utils import gen_grid_up
    from models.vrcnet import Folding
    mod = Folding(4, 4, r, 4)
    assert tuple(mod.grid.shape) == (r, 2)
    assert torch.equal(mod.grid.t(), gen_grid_up(r, 0.2))
    assert torch.equal(mod.grid, D.grid_up(r))
    assert np.array_equal(mod.grid.numpy(), gold[f"grid/{r}"])
    assert "grid" not in mod.state_dict()


def test_modules_construct_with_the_reference_state_dict(gold):
    from chamfer3D.model_utils import EF_expansion
    from models import vrcnet as M
    E, Fo = D.EF, D.FOLD
    cases = {"ef": EF_expansion(E["C"], E["O"], E["r"], E["k"]),
             "fold": M.Folding(Fo["C"], Fo["output_size"], Fo["step_ratio"], Fo["G"])}
    for name, c in D.DECS.items():
        cases[name] = M.MSAP_SKN_decoder(c["num_coarse_raw"], c["num_fps"], c["num_coarse"], c["num_fine"], c["layers"],
                                         c["knn_list"], c["pk"], c["points_label"], c["local_folding"], c["over_scale"],
                                         pts_num=c["pts_num"])
    for name, mod in cases.items():
        sd = mod.state_dict()
        assert list(sd) == list(gold[f"{name}/keys"]), name
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(gold[f"{name}/shapes"]), name
        Pr = D.fixture(name)[0]
        assert list(Pr) == list(sd)
        mod.load_state_dict(Pr, strict=True)
    assert cases["ef"].conv1.weight.dim() == 4
    assert cases["dec_fold"].expansion1 is None and cases["dec_ef"].expansion1.step_ratio == 2
    assert cases["dec_ef"].expansion2.step_ratio == 3 and cases["dec_fold"].encoder.pts_num == D.DEC_FOLD["pts_num"]
    assert M.MSAP_SKN_decoder(1024, 2048, 1024, 2048, [1, 1, 1, 1], [16], 10, True, True).encoder.pts_num == [3072, 1536, 768, 384]
    with pytest.raises(ValueError, match="num_models"):
        M.Folding(8, 16, 2, 24, num_models=2)


def test_get_graph_feature_is_there_for_parity_only():
    import inspect
    from chamfer3D import model_utils as U
    assert list(inspect.signature(U.get_graph_feature).parameters) == ["x", "k", "minus_center"]
    assert "get_graph_feature(" not in inspect.getsource(U.EF_expansion)


def test_bad_arguments_raise_before_device_work():
    from chamfer3D.model_utils import EF_expansion
    from models import vrcnet as M
    from ured_hip.vrc import EfEdgeFn, EfMaxFn, FoldFn
    with pytest.raises(ValueError, match="k 33"):
        EF_expansion(16, 8, 2, k=33)
    with pytest.raises(ValueError, match="input_size"):
        EF_expansion(513, 8, 2)
    with pytest.raises(ValueError, match="output_size"):
        EF_expansion(16, 257, 2)
    with pytest.raises(ValueError, match="step_ratio"):
        EF_expansion(16, 8, 17)
    with pytest.raises(ValueError, match="step_ratio"):
        M.Folding(8, 16, 17, 24)
    ef = EF_expansion(16, 8, 2, 4)
    with pytest.raises(TypeError, match="int32"):
        ef.core_rows(torch.zeros(2 * 8, 16), torch.zeros(2, 8, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="exceeds the cloud"):
        EfEdgeFn.apply(torch.zeros(2 * 3, 16), torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="halves"):
        EfEdgeFn.apply(torch.zeros(2 * 8, 15), torch.zeros(2, 8, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="step ratio"):
        EfMaxFn.apply(torch.zeros(8 * 4 * 17, 8), 1, 8, 4, 17)
    with pytest.raises(ValueError, match="O 257"):
        EfMaxFn.apply(torch.zeros(8 * 4 * 2, 257), 1, 8, 4, 2)
    with pytest.raises(ValueError, match="step ratio"):
        FoldFn.apply(torch.zeros(4, 8), torch.zeros(17, 8))
    dec = M.MSAP_SKN_decoder(24, 32, 16, 32, [1, 1, 1, 1], [4, 8], 4, True, True, pts_num=[64, 32, 16, 8])
    with pytest.raises(ValueError, match="global_feat"):
        dec(torch.zeros(2, 512), torch.zeros(2, 3, 40))
    with pytest.raises(ValueError, match="point_input"):
        dec(torch.zeros(2, 1024), torch.zeros(2, 4, 40))
    # with valid arguments the first thing that fails without a GPU is the device requirement
    with pytest.raises(RuntimeError, match="MI355X"):
        EfEdgeFn.apply(torch.zeros(2 * 8, 16), torch.zeros(2, 8, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="MI355X"):
        FoldFn.apply(torch.zeros(4, 8), torch.zeros(2, 8))


def test_c_entry_points_validate_before_device_work(built):
    from ured_hip import _lib
    import ured_hip.vrc  # noqa: F401  (binds the entry points)
    with pytest.raises(_lib.UredError, match="bad sizes"):
        _lib.call("ured_vrc_ef_edge_fwd", None, None, None, -1, 8, 4, 8, None, None)
    with pytest.raises(_lib.UredError, match="k 33"):
        _lib.call("ured_vrc_ef_edge_fwd", None, None, None, 1, 64, 33, 8, None, None)
    with pytest.raises(_lib.UredError, match="exceeds the cloud"):
        _lib.call("ured_vrc_ef_edge_bwd", None, None, None, 1, 3, 4, 8, None, None, None)
    with pytest.raises(_lib.UredError, match="width 4097"):
        _lib.call("ured_vrc_ef_edge_bwd", None, None, None, 1, 8, 4, 4097, None, None, None)
    with pytest.raises(_lib.UredError, match="bad sizes"):
        _lib.call("ured_vrc_ef_max_fwd", None, 1, -8, 4, 2, 8, None, None, None)
    with pytest.raises(_lib.UredError, match="k 33"):
        _lib.call("ured_vrc_ef_max_bwd", None, None, 1, 64, 33, 2, 8, None, None)
    with pytest.raises(_lib.UredError, match="step ratio 17"):
        _lib.call("ured_vrc_ef_max_fwd", None, 1, 8, 4, 17, 8, None, None, None)
    with pytest.raises(_lib.UredError, match="exceeds 2\\^31"):
        _lib.call("ured_vrc_ef_max_fwd", None, 65535, 4096, 4, 2, 8, None, None, None)
    with pytest.raises(_lib.UredError, match="bad sizes"):
        _lib.call("ured_vrc_fold_fwd", None, None, 1, 8, 2, -4, None, None)
    with pytest.raises(_lib.UredError, match="step ratio 17"):
        _lib.call("ured_vrc_fold_bwd", None, None, 1, 8, 17, 4, 32, None, None, None)
    with pytest.raises(_lib.UredError, match="chunk"):
        _lib.call("ured_vrc_fold_bwd", None, None, 1, 8, 2, 4, 0, None, None, None)
    with pytest.raises(_lib.UredError, match="null pointer"):
        _lib.call("ured_vrc_fold_fwd", None, None, 1, 8, 2, 4, None, None)
