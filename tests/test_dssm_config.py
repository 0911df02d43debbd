"""`dssm {...}` from its config (tests/golden/dssm_mini.config and its in-batch variant, tests/dssm_variants.py) on the lane
emulator: the model builds with the reference's parameter names; the fused head and the literal form agree; two training steps
move both towers' tables and every dense parameter; everything the model does not build is refused by name."""
import os

import pytest
import torch

import dssm_variants as dv
from torcheasyrec_amd import _lib, match
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.rank_model import _MODELS, build_rank_model

# tzrec/models/dssm.py:86-135 over the mini config: per tower its embedding group's tables, `mlp.mlp.<i>.perceptron.0` of a
# [16, 8] MLP (this package's `mlp.mlp.<2i>`, tests/test_dssm_reference_vectors.py) and `output`
REFERENCE_KEYS = sorted(
    [f"user_tower.embedding_group.ebc.embedding_bags.{t}.weight" for t in ("user_id_emb", "age_level_emb")]
    + [f"item_tower.embedding_group.ebc.embedding_bags.{t}.weight" for t in ("adgroup_id_emb", "cate_id_emb")]
    + [f"{t}.{m}.{p}" for t in ("user_tower", "item_tower") for m in ("mlp.mlp.0", "mlp.mlp.2", "output") for p in ("weight", "bias")])


@pytest.fixture
def emu(emu_path):
    _lib.use_library(emu_path)
    return torch.device("cpu")


def build(text, seed=0, **kw):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=torch.device("cpu"), **kw)


@pytest.mark.parametrize("variant", ["sampled", "in_batch"])
def test_builds_with_the_references_names(emu, variant):
    spec, model = build(dv.TEXT if variant == "sampled" else dv.in_batch())
    assert type(model) is _MODELS["dssm"] is match.ConfigDSSM
    assert sorted(model.state_dict()) == REFERENCE_KEYS
    assert (spec.negative_sampler is not None) == (variant == "sampled")
    if variant == "sampled":
        assert spec.negative_sampler["num_sample"] == 12 and spec.negative_sampler["attr_fields"] == ["adgroup_id", "cate_id", "price"]
        assert spec.negative_sampler["item_id_field"] == "adgroup_id" and spec.sampler_kinds == ["negative_sampler"]
    assert model.item_tower.embedding_group._data_group == ("__NEG__" if variant == "sampled" else "__BASE__")
    assert model.user_tower.embedding_group._data_group == "__BASE__"
    assert len(model.fused_optimizers) == 2 and model.fused_optimizers[0] is not model.fused_optimizers[1]
    dense = {id(p) for p in model.dense_parameters()}
    assert dense == {id(p) for n, p in model.named_parameters() if ".embedding_group." not in n} and len(dense) == 12
    b = dv.batches(spec, 9, 1)[0]
    out = model(b)
    assert out["similarity"].shape == ((9, 13) if variant == "sampled" else (9, 9)) and out["rank"].shape == (9,)


def float64_twin(model, b, weights):
    """the model's dense half and head in float64 on the SAME embedding-group outputs: per tower relu(Linear) layers and the output
    Linear over double copies of its parameters, the literal normalize / sim / cross_entropy form -> kind -> [tensor]"""
    import torch.nn.functional as F

    params, embs = {}, []
    for t in ("user_tower", "item_tower"):
        tower = getattr(model, t)
        with torch.no_grad():
            h = tower.build_input(b)[tower._group_name].double()
        for n, p in tower.named_parameters():
            if not n.startswith("embedding_group."):
                params[f"{t}.{n}"] = p.detach().double().clone().requires_grad_(True)
        lins = tower.mlp.linears()
        names = [n for n, m in tower.mlp.named_modules() if any(m is l for l in lins)]
        assert len(names) == len(lins) == 2
        for n in names:
            h = torch.relu(F.linear(h, params[f"{t}.mlp.{n}.weight"], params[f"{t}.mlp.{n}.bias"]))
        embs.append(F.linear(h, params[f"{t}.output.weight"], params[f"{t}.output.bias"]))
    sim = match.match_scores(embs[0], embs[1], model._mode, model._cosine, model._temperature)
    loss = match.scores_loss_rank(sim, model._mode, model._weights(b).double() if weights else None)[0]
    grads = torch.autograd.grad(loss, [params[n] for n in sorted(params)])
    return {"loss": [loss.detach()], "sim": [sim.detach()], "gparam": list(grads)}


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("variant", ["sampled", "in_batch"])
def test_fused_and_literal_heads_agree(emu, monkeypatch, variant, weights):
    """`loss_and_predictions` under FUSED_MATCH_SOFTMAX True and False within the kernel's bound (tests/test_match_softmax.py):
    per kind (loss, similarity, the twelve dense parameter gradients) max |got - fp64| / max(1, |fp64|) of the fused form at or
    below 4 x the same distance of the literal fp32 form, floor 2^-20, against a float64 twin of the towers' dense half and the
    head on the same embedding-group outputs; equal rank"""
    from mlp_ref import check, rel_err

    text = dv.TEXT if variant == "sampled" else dv.in_batch()
    if weights:
        text = dv.with_line(text, '    label_fields: "clk"\n', '    sample_weight_fields: "w"\n')
    res, want = {}, None
    for fused in (True, False):  # identically seeded twins: a backward applies the fused sparse update to the tables
        spec, model = build(text)
        b = dv.batches(spec, 33, 1, seed=2, weights=weights)[0]
        if want is None:
            want = float64_twin(model, b, weights)
        monkeypatch.setattr(match, "FUSED_MATCH_SOFTMAX", fused)
        model.want_similarity = True
        calls, L = [], _lib.lib()
        orig = L.tzr_match_softmax_fwd
        L.tzr_match_softmax_fwd = lambda *a: (calls.append(1), orig(*a))[1]
        try:
            losses, preds = model.loss_and_predictions(b)
        finally:
            L.tzr_match_softmax_fwd = orig
        assert len(calls) == (1 if fused else 0) and sorted(losses) == ["softmax_cross_entropy"] and sorted(preds) == ["rank", "similarity"]
        losses["softmax_cross_entropy"].backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        assert len(grads) == 12 and all(".embedding_group." not in n for n in grads)
        res[fused] = ({"loss": [losses["softmax_cross_entropy"].detach()], "sim": [preds["similarity"].detach()],
                       "gparam": [grads[n] for n in sorted(grads)]}, preds["rank"])
        model.want_similarity = False
        with torch.no_grad():
            assert sorted(model.loss_and_predictions(b)[1]) == ["rank"]
    kinds = ("loss", "sim", "gparam")
    gaps = {k: rel_err(res[False][0][k], want[k]) for k in kinds}
    check(res[True][0], want, gaps, f"dssm {variant} weights={weights}", kinds)
    assert torch.equal(res[True][1], res[False][1])


@pytest.mark.parametrize("variant", ["sampled", "in_batch"])
def test_two_training_steps_move_both_towers(emu, variant):
    from torcheasyrec_amd.embedding_group import TrainPipeline

    spec, model = build(dv.TEXT if variant == "sampled" else dv.in_batch())
    opt = torch.optim.Adam(list(model.dense_parameters()), lr=1e-2)
    before_t = {f"{t}/{n}": w.detach().clone() for t in ("user_tower", "item_tower")
                for n, w in getattr(model, t).embedding_group.ebc.table_weights().items()}
    before_p = {n: p.detach().clone() for n, p in model.named_parameters() if ".embedding_group." not in n}
    pipe = TrainPipeline(model, opt, torch.device("cpu"), model.loss)
    it, seen = iter(dv.batches(spec, 16, 2, seed=5)), []
    for _ in range(2):
        losses, preds, _ = pipe.progress(it)
        seen.append(float(losses["softmax_cross_entropy"].detach()))
        assert sorted(preds) == ["rank"]  # (the pipeline took loss_and_predictions: no score matrix)
    assert all(torch.isfinite(torch.tensor(seen)))
    after_t = {f"{t}/{n}": w.detach() for t in ("user_tower", "item_tower") for n, w in getattr(model, t).embedding_group.ebc.table_weights().items()}
    assert len(before_t) == 4
    for n in before_t:
        assert not torch.equal(before_t[n], after_t[n]), n
    for n, p in model.named_parameters():
        if n in before_p:
            assert not torch.equal(before_p[n], p.detach()), n


def test_evaluate_returns_recall_in_order(emu):
    from torcheasyrec_amd.metrics import Evaluator, evaluate

    for text in (dv.TEXT, dv.in_batch()):
        spec, model = build(text)
        out = evaluate(model, dv.batches(spec, 16, 3, seed=6), Evaluator(model, spec, torch.device("cpu")))
        assert sorted(out) == ["recall@1", "recall@5"] and 0.0 <= float(out["recall@1"]) <= float(out["recall@5"]) <= 1.0


SAMPLER_BLOCK = '    {kind} {{ input_path: "t" num_sample: 4 attr_fields: "adgroup_id" item_id_field: "adgroup_id" }}\n'
DATA_ANCHOR = "    num_workers: 1\n"
MODEL_ANCHOR = "    losses { softmax_cross_entropy {} }\n"
REFUSALS = {
    "hard_negative_sampler": (lambda t: dv.with_line(t.replace(dv.SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="hard_negative_sampler")), NotImplementedError),
    "hard_negative_sampler_v2": (lambda t: dv.with_line(t.replace(dv.SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="hard_negative_sampler_v2")), NotImplementedError),
    "negative_sampler_v2": (lambda t: dv.with_line(t.replace(dv.SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="negative_sampler_v2")), NotImplementedError),
    "tdm_sampler": (lambda t: dv.with_line(t.replace(dv.SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="tdm_sampler")), NotImplementedError),
    "variational_dropout": (lambda t: dv.with_line(t, MODEL_ANCHOR, "    variational_dropout { regularization_lambda: 0.01 }\n"), NotImplementedError),
    "train_metrics": (lambda t: dv.with_line(t, MODEL_ANCHOR, "    train_metrics { recall_at_k { top_k: 1 } }\n"), NotImplementedError),
    "softmax_cross_entropy": (lambda t: t.replace(MODEL_ANCHOR, "    losses { binary_cross_entropy {} }\n"), ValueError),
    "exactly one loss": (lambda t: dv.with_line(t, MODEL_ANCHOR, MODEL_ANCHOR), ValueError),
    "recall_at_k only": (lambda t: dv.with_line(t, MODEL_ANCHOR, "    metrics { auc {} }\n"), ValueError),
    "in_batch_negative": (lambda t: dv.with_line(t, "        temperature: 0.05\n", "        in_batch_negative: true\n"), ValueError),
    "'cate_id_emb' appears in both": (lambda t: dv.with_line(t, '        feature_names: "age_level"\n', '        feature_names: "cate_id"\n'), NotImplementedError),
    "zch": (lambda t: t.replace('feature_name: "user_id" num_buckets: 500 embedding_dim: 16',
                                'feature_name: "user_id" embedding_dim: 16 zch { zch_size: 128 eviction_interval: 2 lfu {} }'), NotImplementedError),
    "no field 'num_towers'": (lambda t: dv.with_line(t, "        output_dim: 8\n", "        num_towers: 2\n"), ValueError),
    "user_tower has no field 'dropout'": (lambda t: t.replace('user_tower { input: "user" mlp', 'user_tower { input: "user" dropout: 1 mlp'), ValueError),
    "similarity 'EUCLID'": (lambda t: t.replace("similarity: COSINE", "similarity: EUCLID"), ValueError),
    "needs `output_dim`": (lambda t: t.replace("        output_dim: 8\n", ""), ValueError),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refused_by_name_when_the_model_is_built(emu, name):
    make, exc = REFUSALS[name]
    text = make(dv.TEXT)
    assert text != dv.TEXT
    with pytest.raises(exc, match=name.split("'")[1] if "'" in name else name) as e:
        build(text)
    assert "dssm" in str(e.value)


def test_sharded_towers_are_refused(emu):
    with pytest.raises(NotImplementedError, match="process_group"):
        build(dv.TEXT, process_group=object())


def test_softmax_cross_entropy_with_one_class_still_needs_a_match_model():
    """the refusal for rank models, word for word"""
    text = open(os.path.join(dv.GOLDEN, "deepfm_mini.config")).read()
    assert text.count("    losses { binary_cross_entropy {} }\n") == 1
    with pytest.raises(ValueError, match=r"^model_config: num_class must be greater than 1 when loss type is softmax_cross_entropy \(got 1\)$"):
        load_pipeline_spec(text.replace("    losses { binary_cross_entropy {} }\n", "    losses { softmax_cross_entropy {} }\n"))
    assert load_pipeline_spec(dv.TEXT).losses[0].kind == "softmax_cross_entropy"  # (and the match model's parses)
