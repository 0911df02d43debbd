"""`dbmtl {...}` from its config (tests/golden/dbmtl_mini.config): the model the reference builds from the same file
(tzrec/models/dbmtl.py:28-175) with its parameter names, the refusals, and the relation towers on csrc/relation_chain.hip
against the literal cat / MLP form on the same weights."""
import pytest
import torch

import relation_chain_ref as ref
from cross_v2_ref import FLOOR, rel_err
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import _lib, rank_model
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.dense import FusedDenseAdam
from torcheasyrec_amd.metrics import Evaluator, evaluate
from torcheasyrec_amd.rank_model import ConfigDBMTL, MultiTaskRankModel, build_rank_model

from dbmtl_variants import TEXT, with_sequence
BOTTOM = "        bottom_mlp { hidden_units: [32] }\n"
LOSSES = ["binary_cross_entropy_ctr", "binary_cross_entropy_cvr", "binary_cross_entropy_pay"]
MASK = "        mask_net { n_mask_blocks: 2 mask_block { reduction_ratio: 2.0 hidden_dim: 24 } top_mlp { hidden_units: [40] } }\n"


def _model(dev, seed=0, text=TEXT):
    assert TEXT.count(BOTTOM) == 1
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=dev)


@pytest.fixture
def fwd_calls():
    calls = {"n": 0, "lib": None, "orig": None}

    def arm():
        L = _lib.lib()
        calls["lib"], calls["orig"] = L, L.tzr_relation_chain_fwd

        def counted(*a):
            calls["n"] += 1
            return calls["orig"](*a)

        L.tzr_relation_chain_fwd = counted
        return calls

    yield arm
    if calls["lib"] is not None:
        calls["lib"].tzr_relation_chain_fwd = calls["orig"]


def test_config_builds_the_references_model(dev):
    spec, model = _model(dev)
    assert spec.model_name == "dbmtl" and type(model) is ConfigDBMTL and isinstance(model, MultiTaskRankModel)
    d_in = model.embedding_group.group_total_dim("all")
    assert d_in == 16 * 3 + 1  # three ids and price
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.startswith("embedding_group.")}
    want = {"bottom_mlp.mlp.0": (32, d_in),
            "task_mlps.ctr.mlp.0": (16, 32), "task_mlps.ctr.mlp.2": (8, 16),
            "task_mlps.cvr.mlp.0": (16, 32), "task_mlps.cvr.mlp.2": (12, 16),
            "task_mlps.pay.mlp.0": (8, 32),
            "relation_mlps.cvr.mlp.0": (16, 12 + 8), "relation_mlps.cvr.mlp.2": (8, 16),  # [cvr's own 12 | ctr's 8]
            "relation_mlps.pay.mlp.0": (12, 8 + 8 + 8),                                    # [pay's own 8 | ctr's 8 | cvr's relation 8]
            "task_outputs.0": (1, 8), "task_outputs.1": (1, 8), "task_outputs.2": (1, 12)}
    full = {}
    for k, s in want.items():
        full[k + ".weight"], full[k + ".bias"] = s, s[:1]
    assert shapes == full
    assert isinstance(model.task_mlps, torch.nn.ModuleDict) and isinstance(model.relation_mlps, torch.nn.ModuleDict)
    assert list(model.relation_mlps) == ["cvr", "pay"] and model._relations == [[], [0], [0, 1]]
    assert model.mask_net is None and model.mmoe is None


VARIANTS = {
    "mask_net": (TEXT.replace(BOTTOM, MASK + BOTTOM), 1),
    "mmoe": (TEXT.replace(BOTTOM, BOTTOM + "        expert_mlp { hidden_units: [24, 16] }\n        gate_mlp { hidden_units: [8] }\n"), 1),
    "no_bottom": (TEXT.replace(BOTTOM, ""), 1),
    "sequence": (with_sequence(), 1),  # the dbmtl_has_sequence style: a click history inside the DEEP group, a din_encoder over it
    "no_tower_mlp": (TEXT.replace(" mlp { hidden_units: [16, 8] }", "").replace(" mlp { hidden_units: [16, 12] }", "").replace(" mlp { hidden_units: [8] }", ""), 1),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_build_and_train_two_steps(dev, fwd_calls, name):
    text, per_step = VARIANTS[name]
    calls = fwd_calls()
    spec, model = _model(dev, seed=2, text=text)
    assert (model.mask_net is not None) == (name == "mask_net") and (model.mmoe is not None) == (name == "mmoe")
    assert (model.bottom_mlp is not None) == (name != "no_bottom") and (len(model.task_mlps) == 0) == (name == "no_tower_mlp")
    if name == "mmoe":
        assert model.mmoe.num_expert == 3 and model.mmoe.has_gate_mlp and "mmoe.gate_mlps.2.mlp.0.weight" in model.state_dict()
    if name == "mask_net":
        assert model.bottom_mlp.mlp[0].in_features == 40 and "mask_net.ln_emb.weight" in model.state_dict()
    if name == "sequence":  # the existing embedding group: the din_encoder's output over two 16-wide sequence features joins the group
        assert model.embedding_group.jagged_sequence_groups == {"click_seq"} and model.bottom_mlp.mlp[0].in_features == 16 * 3 + 1 + 32
    if name == "no_tower_mlp":  # every tower reads the bottom MLP's one tensor; ctr's relation output is that tensor itself
        assert model.relation_mlps["cvr"].mlp[0].in_features == 64 and model.relation_mlps["pay"].mlp[0].in_features == 32 + 32 + 8
    opt = FusedDenseAdam(list(model.dense_parameters()), lr=0.01)
    batch = next(synthetic_batches(spec, 40, 40, seed=3)).to(dev)
    for _ in range(2):
        loss = model.loss(model(batch), batch)
        assert sorted(loss) == LOSSES
        opt.zero_grad()
        sum(loss.values()).backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.dense_parameters())
        opt.step()
    assert calls["n"] == 2 * per_step  # the whole chain: one forward launch per step
    assert all(bool(torch.isfinite(v).all()) for v in model(batch).values())


def test_configs_the_reference_cannot_run_are_refused(dev):
    later = TEXT.replace('relation_tower_names: "ctr"\n            relation_mlp { hidden_units: [16, 8] }', 'relation_tower_names: "pay"\n            relation_mlp { hidden_units: [16, 8] }')
    assert later != TEXT
    with pytest.raises(ValueError, match="'cvr'.*relation_tower_names.*'pay'.*later"):
        _model(dev, text=later)
    with pytest.raises(ValueError, match="'pay'.*relation_tower_names.*'buy'"):
        _model(dev, text=TEXT.replace('relation_tower_names: "cvr"', 'relation_tower_names: "buy"'))
    with pytest.raises(ValueError, match="'pay'.*relation_tower_names.*itself"):
        _model(dev, text=TEXT.replace('relation_tower_names: "cvr"', 'relation_tower_names: "pay"'))
    with pytest.raises(ValueError, match="tower_name.*'ctr'.*twice"):
        _model(dev, text=TEXT.replace('tower_name: "pay"', 'tower_name: "ctr"'))
    with pytest.raises(ValueError, match="dbmtl has no field 'extraction_networks'"):
        _model(dev, text=TEXT.replace(BOTTOM, BOTTOM + "        extraction_networks { network_name: \"a\" }\n"))
    with pytest.raises(ValueError, match="'pay' has no field 'relation_names'"):
        _model(dev, text=TEXT.replace('relation_tower_names: "cvr"', 'relation_names: "cvr"'))
    with pytest.raises(NotImplementedError, match="'pay'.*pareto_min_loss_weight"):
        _model(dev, text=TEXT.replace('tower_name: "pay"', 'tower_name: "pay" pareto_min_loss_weight: 0.1'))
    with pytest.raises(NotImplementedError, match="'pay'.*train_metrics"):
        _model(dev, text=TEXT.replace('tower_name: "pay"', 'tower_name: "pay" train_metrics { auc {} }'))
    # what the reference runs: names without a relation MLP are ignored; a relation MLP without names reads the tower's own output
    _, m = _model(dev, text=TEXT.replace("            relation_mlp { hidden_units: [12] }\n", ""))
    assert list(m.relation_mlps) == ["cvr"] and m._relations[2] == [] and m.task_outputs[2].in_features == 8
    _, m = _model(dev, text=TEXT.replace('            relation_tower_names: "ctr"\n            relation_mlp { hidden_units: [16, 8] }', "            relation_mlp { hidden_units: [16, 8] }"))
    assert m.relation_mlps["cvr"].mlp[0].in_features == 12 and m._relations[1] == []


def _grads(dev, fused, monkeypatch, text=TEXT):
    monkeypatch.setattr(rank_model, "FUSED_RELATION_CHAIN", fused)
    spec, model = _model(dev, seed=3, text=text)
    batch = next(synthetic_batches(spec, 96, 96, seed=4)).to(dev)
    out = model(batch)
    loss = model.loss(out, batch)
    sum(loss.values()).backward()
    names = [n for n, _ in model.named_parameters()
             if not n.startswith("embedding_group.") or n.startswith("embedding_group._group_name_to_seq_encoders.")]  # (dense_parameters())
    assert len(names) == len(list(model.dense_parameters()))
    return ([out[k].detach().cpu() for k in sorted(out) if k.startswith("logits")],
            {n: p.grad.detach().cpu() for n, p in model.named_parameters() if n in names})


@pytest.mark.parametrize("name", ["mini", "no_tower_mlp", "sequence"])
def test_fused_and_literal_agree_on_the_same_weights(dev, monkeypatch, fwd_calls, name):
    """forward and every dense gradient with FUSED_RELATION_CHAIN on and off, one seed, one batch.  The bound is the kernel
    test's: 4 x the fp32 literal form's distance to float64, floor 2^-20, relative to max(1, |value|) -- the gap measured on a
    relation chain of the model's shape (tests/relation_chain_ref.py), the largest of its kinds."""
    text = TEXT if name == "mini" else VARIANTS[name][0]
    calls = fwd_calls()
    ya, ga = _grads(dev, True, monkeypatch, text)
    assert calls["n"] == 1
    yb, gb = _grads(dev, False, monkeypatch, text)
    assert calls["n"] == 1  # the literal run never calls the kernel
    xs, layers, gouts = ref.draw(96, [8, 12, 8], [[], [0], [0, 1]], [[], [16, 8], [12]], seed=1)
    gap = max(ref.gaps(xs, [[], [0], [0, 1]], layers, gouts, ref.literal(xs, [[], [0], [0, 1]], layers, gouts)).values())
    bound = max(4.0 * gap, FLOOR)
    err_y = rel_err(ya, [y.double() for y in yb])
    err_g = max(rel_err([ga[n]], [gb[n].double()]) for n in ga)
    print(f"{name} fused vs literal on {dev.type}: logits {err_y:.3e} gradients {err_g:.3e} bound {bound:.3e}")
    assert sorted(ga) == sorted(gb) and len(ga) >= 12
    assert err_y <= bound and err_g <= bound


def test_losses_fall_over_30_steps(dev):
    spec, model = _model(dev, seed=5)
    opt = FusedDenseAdam(list(model.dense_parameters()), lr=0.01)
    batch = next(synthetic_batches(spec, 128, 128, seed=6)).to(dev)
    hist = []
    for _ in range(30):
        loss = model.loss(model(batch), batch)
        opt.zero_grad()
        sum(loss.values()).backward()
        opt.step()
        hist.append([float(loss[k].detach()) for k in LOSSES])
    print("first", hist[0], "last", hist[-1])
    assert all(hist[-1][i] < hist[0][i] for i in range(3))


def test_evaluator_returns_an_auc_per_tower(dev):
    spec, model = _model(dev, seed=7)
    batches = list(synthetic_batches(spec, 2 * 64 + 5, 64, seed=8))
    got = evaluate(model, iter(batches), Evaluator(model, spec, dev))
    assert sorted(got) == ["auc_ctr", "auc_cvr", "auc_pay"] and all(0.0 <= float(v) <= 1.0 for v in got.values())
