"""`mind {...}` from its config (tests/golden/mind_mini.config) on the lane emulator: the model builds with the reference's
parameter names; the fused kernels (capsule layer, label-aware attention, similarity head) and the literal forms agree; a few
training steps through the example's batches move every table and every dense parameter and recall@k is reported; everything the
model does not build is refused by name."""
import copy
import os
import re
import sys

import pytest
import torch

import mind_variants as mv
from torcheasyrec_amd import _lib, capsule, match
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.rank_model import _MODELS, build_rank_model

# tzrec/models/mind.py:67-141, 229-232 over the mini config, the reference's `mlp.<i>.perceptron.0` being this package's `mlp.<2i>`
# (tests/test_mind_reference_vectors.py loads them by these names); each tower's embedding group's tables beside them
REFERENCE_DENSE_KEYS = [
    "user_tower.user_mlp.mlp.0.perceptron.0.weight", "user_tower.user_mlp.mlp.0.perceptron.0.bias",
    "user_tower.user_mlp_out.weight", "user_tower.user_mlp_out.bias",
    "user_tower._hist_seq_mlp.mlp.0.perceptron.0.weight", "user_tower._hist_seq_mlp_out.weight",
    "user_tower._capsule_layer.bilinear_matrix",
    "user_tower._concat_mlp.mlp.0.perceptron.0.weight", "user_tower._concat_mlp.mlp.0.perceptron.0.bias",
    "user_tower._concat_mlp.mlp.1.perceptron.0.weight", "user_tower._concat_mlp.mlp.1.perceptron.0.bias",
    "user_tower.output.weight",
    "item_tower.mlp.mlp.0.perceptron.0.weight", "item_tower.mlp.mlp.0.perceptron.0.bias",
    "item_tower.mlp.mlp.1.perceptron.0.weight", "item_tower.mlp.mlp.1.perceptron.0.bias",
    "item_tower.output.weight", "item_tower.output.bias"]
TABLE_KEYS = ["user_tower.embedding_group.ebc.embedding_bags.user_id_emb.weight", "user_tower.embedding_group.ebc.embedding_bags.age_level_emb.weight",
              "user_tower.embedding_group.ecs.16._store.embedding_bags.click_seq__adgroup_id_emb.weight",
              "user_tower.embedding_group.ecs.8._store.embedding_bags.click_seq__cate_id_emb.weight",
              "item_tower.embedding_group.ebc.embedding_bags.adgroup_id_emb.weight", "item_tower.embedding_group.ebc.embedding_bags.cate_id_emb.weight"]


def _ours(ref_key):
    return re.sub(r"mlp\.(\d+)\.perceptron\.0\.", lambda m: f"mlp.{2 * int(m.group(1))}.", ref_key)


@pytest.fixture
def emu(emu_path):
    _lib.use_library(emu_path)
    return torch.device("cpu")


def build(text, seed=0, **kw):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=torch.device("cpu"), **kw)


def test_builds_with_the_references_names(emu):
    spec, model = build(mv.TEXT)
    assert type(model) is _MODELS["mind"] is match.ConfigMIND and isinstance(model, match.ConfigMatchModel)
    assert issubclass(match.ConfigDSSM, match.ConfigMatchModel)  # (one base, no second copy of the plumbing)
    assert sorted(model.state_dict()) == sorted([_ours(k) for k in REFERENCE_DENSE_KEYS] + TABLE_KEYS)
    ut = model.user_tower
    assert ut.embedding_group.jagged_sequence_groups == {"hist"} and ut.embedding_group._data_group == "__BASE__"
    assert model.item_tower.embedding_group._data_group == "__NEG__"
    assert ut._capsule_layer.cfg == capsule.CapsuleConfig(max_k=3, max_seq_len=20, high_dim=8, num_iters=3)  # (the proto's defaults behind them)
    assert model._simi_pow == 10.0 and model._cosine and not model._head_cosine and model._temperature == 0.05
    dense = {id(p) for p in model.dense_parameters()}
    assert dense == {id(p) for n, p in model.named_parameters() if ".embedding_group." not in n} and len(dense) == 18
    assert len(model.fused_optimizers) == 2
    b = mv.batches(spec, 9, 1)[0]
    out = model(b)
    assert out["similarity"].shape == (9, 13) and out["rank"].shape == (9,)
    interests, mask = ut(b)
    assert interests.shape == (9, 3, 8) and mask.shape == (9, 3) and mask.dtype == torch.bool and bool(mask[:, 0].all())
    assert float(interests.detach()[~mask].abs().sum()) == 0.0  # (a masked interest is a zero row, normalized to zero)


def float64_dense_half(model, xu, rows, offsets, logits0, xv):
    """the model's dense half, attention and head in float64 (double inputs take every literal form) on the SAME embedding-group
    outputs -> kind -> [tensor]"""
    twin = copy.deepcopy(model)
    for t in (twin.user_tower, twin.item_tower):
        del t.embedding_group
    twin = twin.double()
    xs = [t.detach().double().requires_grad_(True) for t in (xu, rows, xv)]
    interests, mask = twin.user_tower.interests(xs[0], xs[1], offsets, logits0.double())
    v = twin.item_tower.embed(xs[2])
    u = match.label_attention(interests, v, mask, twin._simi_pow)
    sim = match.match_scores(u, v, twin._mode, False, twin._temperature)
    loss, rank = match.scores_loss_rank(sim, twin._mode)
    params = [p for _, p in sorted(twin.named_parameters())]
    grads = torch.autograd.grad(loss, xs + params)
    return {"loss": [loss.detach()], "sim": [sim.detach()], "gx": list(grads[:3]), "gparam": list(grads[3:])}, rank


@pytest.mark.parametrize("seed", [2, 3])
def test_fused_and_literal_models_agree(emu, monkeypatch, seed):
    """The dense half of the model on the embedding groups' outputs (user features [B, .], history rows [N, .], item rows [M, .])
    with the three kernels on and off, one recorded draw of the routing logits: per kind (loss, similarity, the gradients of
    the three inputs -- the embedding gradients --, the eighteen dense parameter gradients) max |got - fp64| / max(1, |fp64|) of
    the fused form at or below 4 x the same distance of the literal fp32 form, floor 2^-20, against a float64 twin; equal rank
    and mask."""
    from mlp_ref import check, rel_err

    spec, model = build(mv.TEXT)
    b = mv.batches(spec, 33, 1, seed=seed)[0]
    ut, it = model.user_tower, model.item_tower
    with torch.no_grad():
        fu, fi = ut.build_input(b), it.build_input(b)
        rows, offsets = ut.history_rows(fu)
        xu, xv = fu[ut._group_name], fi[it._group_name]
    assert rows.shape[1] == 24 and offsets.shape == (34,) and int(offsets[-1]) == rows.shape[0]
    logits0 = torch.randn(rows.shape[0], 3, generator=torch.Generator().manual_seed(seed))
    want, want_rank = float64_dense_half(model, xu, rows, offsets, logits0, xv)
    names = ("tzr_capsule_fwd", "tzr_label_attn_fwd", "tzr_match_softmax_fwd")
    res = {}
    for fused in (True, False):
        for mod, name in ((match, "FUSED_MATCH_SOFTMAX"), (match, "FUSED_LABEL_ATTENTION"), (capsule, "FUSED_CAPSULE")):
            monkeypatch.setattr(mod, name, fused)
        L = _lib.lib()
        orig, calls = {n: getattr(L, n) for n in names}, []
        for n in names:
            setattr(L, n, (lambda n: lambda *a: (calls.append(n), orig[n](*a))[1])(n))
        try:
            model.zero_grad()
            model.want_similarity = True
            xs = [t.detach().clone().requires_grad_(True) for t in (xu, rows, xv)]
            interests, mask = ut.interests(xs[0], xs[1], offsets, logits0)
            v = it.embed(xs[2])
            losses, preds = model.head(match.label_attention(interests, v, mask, model._simi_pow), v)
            losses["softmax_cross_entropy"].backward()
        finally:
            for n in names:
                setattr(L, n, orig[n])
        assert sorted(calls) == (sorted(names) if fused else [])
        res[fused] = ({"loss": [losses["softmax_cross_entropy"].detach()], "sim": [preds["similarity"].detach()], "gx": [x.grad for x in xs],
                       "gparam": [p.grad.clone() for n, p in sorted(model.named_parameters()) if ".embedding_group." not in n]}, preds["rank"], mask)
    kinds = ("loss", "sim", "gx", "gparam")
    gaps = {k: rel_err(res[False][0][k], want[k]) for k in kinds}
    check(res[True][0], want, gaps, f"mind seed {seed}", kinds)
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])


def test_training_steps_through_the_examples_batches_and_recall(emu):
    """examples/train_from_config.py's own synthetic batches (a click history in the base data group beside the sampler's "__NEG__"
    group) through TrainPipeline, then the config's recall@k"""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "examples"))
    from train_from_config import synthetic_batches

    from torcheasyrec_amd.embedding_group import TrainPipeline
    from torcheasyrec_amd.metrics import Evaluator, evaluate

    spec, model = build(mv.TEXT)
    opt = torch.optim.Adam(list(model.dense_parameters()), lr=1e-2)
    tables = lambda: {n: p.detach().clone() for n, p in model.state_dict().items() if ".embedding_group." in n}  # noqa: E731
    before_t = tables()
    before_p = {n: p.detach().clone() for n, p in model.named_parameters() if ".embedding_group." not in n}
    pipe = TrainPipeline(model, opt, torch.device("cpu"), model.loss)
    calls, L = [], _lib.lib()
    orig = L.tzr_capsule_bwd
    L.tzr_capsule_bwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        it, seen = iter(synthetic_batches(spec, 3 * 16, 16, seed=5)), []
        for _ in range(3):
            losses, preds, _ = pipe.progress(it)
            seen.append(float(losses["softmax_cross_entropy"].detach()))
            assert sorted(preds) == ["rank"]  # (the pipeline took loss_and_predictions: no score matrix)
    finally:
        L.tzr_capsule_bwd = orig
    assert len(calls) == 3 and all(torch.isfinite(torch.tensor(seen)))  # (the capsule kernel trained, not the literal form)
    after_t = tables()
    assert len(before_t) == 6
    for n in before_t:
        assert not torch.equal(before_t[n], after_t[n]), n
    for n, p in model.named_parameters():
        if n in before_p:
            assert not torch.equal(before_p[n], p.detach()), n
    out = evaluate(model, synthetic_batches(spec, 3 * 16, 16, seed=6), Evaluator(model, spec, torch.device("cpu")))
    assert sorted(out) == ["recall@1", "recall@5"] and 0.0 <= float(out["recall@1"]) <= float(out["recall@5"]) <= 1.0


SAMPLER = mv.TEXT[mv.TEXT.index("    negative_sampler {"):mv.TEXT.index("        item_id_field: \"adgroup_id\"\n    }\n") + len("        item_id_field: \"adgroup_id\"\n    }\n")]
SAMPLER_BLOCK = '    {kind} {{ input_path: "t" num_sample: 4 attr_fields: "adgroup_id" item_id_field: "adgroup_id" }}\n'
DATA_ANCHOR = "    num_workers: 1\n"
MODEL_ANCHOR = "    losses { softmax_cross_entropy {} }\n"
CAPSULE = "capsule_config { max_k: 3 max_seq_len: 20 high_dim: 8 num_iters: 3 }"
REFUSALS = {
    # everything ConfigDSSM refuses
    "hard_negative_sampler": (lambda t: mv.with_line(t.replace(SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="hard_negative_sampler")), NotImplementedError),
    "hard_negative_sampler_v2": (lambda t: mv.with_line(t.replace(SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="hard_negative_sampler_v2")), NotImplementedError),
    "negative_sampler_v2": (lambda t: mv.with_line(t.replace(SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="negative_sampler_v2")), NotImplementedError),
    "tdm_sampler": (lambda t: mv.with_line(t.replace(SAMPLER, ""), DATA_ANCHOR, SAMPLER_BLOCK.format(kind="tdm_sampler")), NotImplementedError),
    "variational_dropout": (lambda t: mv.with_line(t, MODEL_ANCHOR, "    variational_dropout { regularization_lambda: 0.01 }\n"), NotImplementedError),
    "train_metrics": (lambda t: mv.with_line(t, MODEL_ANCHOR, "    train_metrics { recall_at_k { top_k: 1 } }\n"), NotImplementedError),
    "softmax_cross_entropy": (lambda t: t.replace(MODEL_ANCHOR, "    losses { binary_cross_entropy {} }\n"), ValueError),
    "exactly one loss": (lambda t: mv.with_line(t, MODEL_ANCHOR, MODEL_ANCHOR), ValueError),
    "recall_at_k only": (lambda t: mv.with_line(t, MODEL_ANCHOR, "    metrics { auc {} }\n"), ValueError),
    "in_batch_negative": (lambda t: mv.with_line(t, "        temperature: 0.05\n", "        in_batch_negative: true\n"), ValueError),
    "'cate_id_emb' appears in both": (lambda t: mv.with_line(t, '        feature_names: "age_level"\n', '        feature_names: "cate_id"\n'), NotImplementedError),
    "zch": (lambda t: t.replace('feature_name: "user_id" num_buckets: 500 embedding_dim: 16',
                                'feature_name: "user_id" embedding_dim: 16 zch { zch_size: 128 eviction_interval: 2 lfu {} }'), NotImplementedError),
    "similarity 'EUCLID'": (lambda t: t.replace("similarity: COSINE", "similarity: EUCLID"), ValueError),
    "needs `output_dim`": (lambda t: t.replace("        output_dim: 8\n", ""), ValueError),
    # MIND's own
    "user_mlp needs at least two hidden_units": (lambda t: t.replace("user_mlp { hidden_units: [16, 8] }", "user_mlp { hidden_units: [8] }"), ValueError),
    "hist_seq_mlp `use_bn`": (lambda t: t.replace("hist_seq_mlp { hidden_units: [16, 12] }", "hist_seq_mlp { hidden_units: [16, 12] use_bn: true }"), NotImplementedError),
    "concat_mlp `use_bn`": (lambda t: t.replace("concat_mlp { hidden_units: [16, 8] }", "concat_mlp { hidden_units: [16, 8] use_bn: true }"), NotImplementedError),
    "no field 'num_interests'": (lambda t: mv.with_line(t, "        simi_pow: 10\n", "        num_interests: 2\n"), ValueError),
    "user_tower has no field 'mlp'": (lambda t: t.replace("            concat_mlp { hidden_units: [16, 8] }\n", "            concat_mlp { hidden_units: [16, 8] }\n            mlp { hidden_units: [8] }\n"), ValueError),
    "item_tower has no field 'history_input'": (lambda t: t.replace('item_tower { input: "item" mlp', 'item_tower { input: "item" history_input: "hist" mlp'), ValueError),
    "capsule_config has no field 'scale_ratio'": (lambda t: t.replace(CAPSULE, CAPSULE[:-1] + "scale_ratio: 1.0 }"), ValueError),
    "capsule_config needs `max_seq_len`": (lambda t: t.replace(CAPSULE, "capsule_config { max_k: 3 high_dim: 8 }"), ValueError),
    "routing_init_method": (lambda t: t.replace(CAPSULE, CAPSULE[:-1] + 'routing_init_method: "uniform" }'), ValueError),
    "history_input 'user' is a DEEP group": (lambda t: t.replace('history_input: "hist"', 'history_input: "user"'), ValueError),
    "history_input 'clicks' is not a feature group": (lambda t: t.replace('history_input: "hist"', 'history_input: "clicks"'), ValueError),
    "user_tower needs `history_input`": (lambda t: t.replace('            history_input: "hist"\n', ""), ValueError),
    "user_tower needs `capsule_config`": (lambda t: t.replace("            " + CAPSULE + "\n", ""), ValueError),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refused_by_name_when_the_model_is_built(emu, name):
    make, exc = REFUSALS[name]
    text = make(mv.TEXT)
    assert text != mv.TEXT
    with pytest.raises(exc, match=re.escape(name.split("'")[1]) if "'" in name else re.escape(name)) as e:
        build(text)
    assert "mind" in str(e.value)


def test_sharded_towers_are_refused(emu):
    with pytest.raises(NotImplementedError, match="process_group"):
        build(mv.TEXT, process_group=object())


def test_user_seq_combine_is_accepted_and_changes_nothing(emu):
    """the reference never reads it"""
    _, a = build(mv.TEXT)
    spec, b = build(mv.TEXT.replace('            history_input: "hist"\n', '            history_input: "hist"\n            user_seq_combine: CONCAT\n'))
    assert sorted(a.state_dict()) == sorted(b.state_dict())
    batch = mv.batches(spec, 9, 1)[0]
    torch.manual_seed(1)
    sa = a(batch)["similarity"]
    torch.manual_seed(1)
    assert torch.equal(sa, b(batch)["similarity"])


def test_a_single_layer_hist_seq_mlp_and_none_build_the_references_keys(emu):
    """mind.py:113-126: one hidden unit: `_hist_seq_mlp` is a Linear without bias; no block: the capsule layer reads the group"""
    _, one = build(mv.TEXT.replace("hist_seq_mlp { hidden_units: [16, 12] }", "hist_seq_mlp { hidden_units: [12] }"))
    keys = [k for k in one.state_dict() if "_hist_seq_mlp" in k]
    assert keys == ["user_tower._hist_seq_mlp.weight"] and one.user_tower._capsule_layer.bilinear_matrix.shape == (12, 8)
    spec, none = build(mv.TEXT.replace("            hist_seq_mlp { hidden_units: [16, 12] }\n", ""))
    assert not [k for k in none.state_dict() if "_hist_seq_mlp" in k] and none.user_tower._capsule_layer.bilinear_matrix.shape == (24, 8)
    losses, _ = none.loss_and_predictions(mv.batches(spec, 9, 1)[0])
    assert bool(torch.isfinite(losses["softmax_cross_entropy"]))
