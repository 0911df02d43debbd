"""`dat {...}` from its config (tests/golden/dat_mini.config and its variants, tests/dat_variants.py) on the lane emulator: the
model builds with the reference's parameter names and one `user_id` lookup feeds two groups; the fused Adaptive-Mimic loss and
the literal form agree, also in the gradient that reaches the augment group; two training steps move both towers' tables and
every dense parameter; everything the model does not build is refused by name."""
import pytest
import torch
import torch.nn.functional as F

import dat_variants as dv
from mlp_ref import check, rel_err
from torcheasyrec_amd import _lib, match
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.rank_model import _MODELS, build_rank_model

# tzrec/models/dat.py:39-166 over the mini config: per tower its embedding group's tables (each once, whatever the number of groups
# that read it), `mlp.mlp.<i>.perceptron.0` of a [24, 16] MLP (this package's `mlp.mlp.<2i>`, tests/test_dat_reference_vectors.py)
# and `output`
REFERENCE_KEYS = sorted(
    [f"user_tower.embedding_group.ebc.embedding_bags.{t}.weight" for t in ("user_id_emb", "age_level_emb")]
    + [f"item_tower.embedding_group.ebc.embedding_bags.{t}.weight" for t in ("adgroup_id_emb", "cate_id_emb")]
    + [f"{t}.{m}.{p}" for t in ("user_tower", "item_tower") for m in ("mlp.mlp.0", "mlp.mlp.2", "output") for p in ("weight", "bias")])
LOSS_KEYS = ["amm_loss_i", "amm_loss_u", "softmax_cross_entropy"]
VARIANTS = ["sampled", "in_batch"]


@pytest.fixture
def emu(emu_path):
    _lib.use_library(emu_path)
    return torch.device("cpu")


def build(text, seed=0, **kw):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=torch.device("cpu"), **kw)


def counted(fn):
    calls, L = [], _lib.lib()
    orig = L.tzr_amm_loss_fwd
    L.tzr_amm_loss_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        return fn(), len(calls)
    finally:
        L.tzr_amm_loss_fwd = orig


def tables(model):
    return {f"{t}/{n}": w.detach().clone() for t in ("user_tower", "item_tower")
            for n, w in getattr(model, t).embedding_group.ebc.table_weights().items()}


@pytest.mark.parametrize("variant", VARIANTS)
def test_builds_with_the_references_names_and_one_lookup_feeds_two_groups(emu, variant):
    spec, model = build(dv.variant(variant))
    assert type(model) is _MODELS["dat"] is match.ConfigDAT
    assert sorted(model.state_dict()) == REFERENCE_KEYS
    assert model.item_tower.embedding_group._data_group == ("__NEG__" if variant == "sampled" else "__BASE__")
    assert len(model.fused_optimizers) == 2 and len(list(model.dense_parameters())) == 12
    for tower, group, aug, key in ((model.user_tower, "user", "user_augment", "user_id"), (model.item_tower, "item", "item_augment", "adgroup_id")):
        eg = tower.embedding_group
        assert sorted(eg.ebc.table_weights()).count(f"{key}_emb") == 1  # one table, one lookup ...
        assert key in eg.group_feature_dims(group) and list(eg.group_feature_dims(aug)) == [key]  # ... read by two groups
        feats = tower.build_input(dv.batches(spec, 9, 1)[0])
        assert torch.equal(feats[group][:, :16], feats[aug]) and feats[aug].shape[1] == tower.embedding_dim() == 16


def float64_twin(model, b, weights):
    """the model's dense half, head and Adaptive-Mimic terms in float64 on the SAME embedding-group outputs: per tower relu(Linear)
    layers and the output Linear over double copies of its parameters on cat([group, augment group]), the literal normalize / sim
    / cross_entropy form and dat.py's AMM expressions -> kind -> [tensor]; "gaug": the gradient of the three losses' sum at the two
    augment groups' outputs, the tower path plus the AMM path"""
    params, embs, augs = {}, [], []
    for t in ("user_tower", "item_tower"):
        tower = getattr(model, t)
        with torch.no_grad():
            feats = tower.build_input(b)
        aug = feats[tower._augment_group_name].double().clone().requires_grad_(True)
        h = torch.cat([feats[tower._group_name].double(), aug], dim=1)
        for n, p in tower.named_parameters():
            if not n.startswith("embedding_group."):
                params[f"{t}.{n}"] = p.detach().double().clone().requires_grad_(True)
        lins = tower.mlp.linears()
        names = [n for n, m in tower.mlp.named_modules() if any(m is l for l in lins)]
        assert len(names) == len(lins) == 2
        for n in names:
            h = torch.relu(F.linear(h, params[f"{t}.mlp.{n}.weight"], params[f"{t}.mlp.{n}.bias"]))
        embs.append(F.linear(h, params[f"{t}.output.weight"], params[f"{t}.output.bias"]))
        augs.append(aug)
    w = model._weights(b).double() if weights else None
    sim = match.match_scores(embs[0], embs[1], model._mode, model._cosine, model._temperature)
    loss = match.scores_loss_rank(sim, model._mode, w)[0]
    lu, li = match.amm_loss_literal(augs[0], augs[1], embs[0], embs[1], model._cosine, model._amm_u, model._amm_i, w)
    grads = torch.autograd.grad(loss + lu + li, [params[n] for n in sorted(params)] + augs)
    return {"loss": [loss.detach()], "amm_u": [lu.detach()], "amm_i": [li.detach()], "gparam": list(grads[:-2]), "gaug": list(grads[-2:])}


def watch_augment(model, seen):
    """the gradient that reaches each tower's augment group output, through a hook on the tensor the embedding group hands out"""
    for t in ("user_tower", "item_tower"):
        tower = getattr(model, t)

        def wrapped(batch, tower=tower, t=t, orig=tower.build_input):
            feats = orig(batch)
            feats[tower._augment_group_name].register_hook(lambda g, t=t: seen.__setitem__(t, g.detach().clone()))
            return feats

        tower.build_input = wrapped


KINDS = ("loss", "amm_u", "amm_i", "gparam", "gaug")


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_and_literal_amm_agree(emu, monkeypatch, variant, weights):
    """`loss_and_predictions` under FUSED_AMM_LOSS True and False within the kernel's bound (tests/test_amm_loss.py): per kind (the
    three losses, the twelve dense parameter gradients, the gradient at the two augment groups' outputs) max |got - fp64| / max(1,
    |fp64|) of the fused form at or below 4 x the same distance of the literal fp32 form, floor 2^-20, against the float64 twin; equal
    rank"""
    text = dv.variant(variant, weights)
    res, want = {}, None
    for fused in (True, False):  # identically seeded twins: a backward applies the fused sparse update to the tables
        spec, model = build(text)
        b = dv.batches(spec, 33, 1, seed=2, weights=weights)[0]
        if want is None:
            want = float64_twin(model, b, weights)
        monkeypatch.setattr(match, "FUSED_AMM_LOSS", fused)
        seen = {}
        watch_augment(model, seen)
        (losses, preds), n = counted(lambda: model.loss_and_predictions(b))
        assert n == (1 if fused else 0) and sorted(losses) == LOSS_KEYS and sorted(preds) == ["rank"]
        sum(losses.values()).backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        assert len(grads) == 12 and all(".embedding_group." not in n for n in grads)
        assert seen["item_tower"].shape[0] == (33 + 12 if variant == "sampled" else 33)
        res[fused] = ({"loss": [losses["softmax_cross_entropy"].detach()], "amm_u": [losses["amm_loss_u"].detach()],
                       "amm_i": [losses["amm_loss_i"].detach()], "gparam": [grads[n] for n in sorted(grads)],
                       "gaug": [seen["user_tower"], seen["item_tower"]]}, preds["rank"])
    gaps = {k: rel_err(res[False][0][k], want[k]) for k in KINDS}
    check(res[True][0], want, gaps, f"dat {variant} weights={weights}", KINDS)
    assert torch.equal(res[True][1], res[False][1])


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_literal_contract_agrees_with_the_fused_one(emu, variant, weights):
    """`loss(forward(b), b)` against `loss_and_predictions(b)`: the same three losses within the bound"""
    spec, model = build(dv.variant(variant, weights))
    b = dv.batches(spec, 33, 1, seed=3, weights=weights)[0]
    want = float64_twin(model, b, weights)
    out = model(b)
    assert sorted(out) == ["item_augment", "item_tower_emb", "rank", "similarity", "user_augment", "user_tower_emb"]
    assert not out["user_tower_emb"].requires_grad and not out["item_tower_emb"].requires_grad and out["user_augment"].requires_grad
    assert torch.allclose(out["user_tower_emb"].norm(dim=1), torch.ones(33), atol=1e-5)  # (COSINE: as the reference's towers deliver them)
    assert out["item_tower_emb"].shape[0] == out["item_augment"].shape[0] == (45 if variant == "sampled" else 33)
    literal = model.loss(out, b)
    (fused, preds), n = counted(lambda: model.loss_and_predictions(b))
    assert n == 1 and sorted(literal) == sorted(fused) == LOSS_KEYS and torch.equal(preds["rank"], out["rank"])
    pick = lambda d: {"loss": [d["softmax_cross_entropy"].detach()], "amm_u": [d["amm_loss_u"].detach()], "amm_i": [d["amm_loss_i"].detach()]}  # noqa: E731
    kinds = ("loss", "amm_u", "amm_i")
    check(pick(fused), want, {k: rel_err(pick(literal)[k], want[k]) for k in kinds}, f"dat literal contract {variant} weights={weights}", kinds)
    with torch.no_grad():
        assert sorted(model(b)) == ["rank", "similarity"]
    model.eval()
    assert sorted(model(b)) == ["rank", "similarity"]
    (losses, _), n = counted(lambda: model.loss_and_predictions(b))
    assert n == 0 and sorted(losses) == ["softmax_cross_entropy"]  # (the reference's towers return no augment vector in eval)
    assert sorted(model.loss(model(b), b)) == ["softmax_cross_entropy"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_training_steps_move_both_towers(emu, variant):
    from torcheasyrec_amd.embedding_group import TrainPipeline

    spec, model = build(dv.variant(variant))
    opt = torch.optim.Adam(list(model.dense_parameters()), lr=1e-2)
    before_t = tables(model)
    before_p = {n: p.detach().clone() for n, p in model.named_parameters() if ".embedding_group." not in n}
    pipe = TrainPipeline(model, opt, torch.device("cpu"), model.loss)
    it = iter(dv.batches(spec, 16, 2, seed=5))
    for _ in range(2):
        (losses, preds, _), n = counted(lambda: pipe.progress(it))
        assert n == 1 and sorted(losses) == LOSS_KEYS and sorted(preds) == ["rank"]  # (the pipeline took loss_and_predictions)
        assert all(bool(torch.isfinite(v.detach())) for v in losses.values())
    after_t = tables(model)
    assert len(before_t) == 4 and len(before_p) == 12
    for n in before_t:
        assert not torch.equal(before_t[n], after_t[n]), n
    for n, p in model.named_parameters():
        if n in before_p:
            assert not torch.equal(before_p[n], p.detach()), n


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_amm_gradient_lands_on_the_augment_tables_rows(emu, variant):
    """the AMM terms alone (no similarity loss) move the two id tables -- read by a group and an augment group of their tower, one
    lookup with two destinations in the fused sparse backward -- and, the embeddings being detached, nothing else"""
    spec, model = build(dv.variant(variant))
    b = dv.batches(spec, 16, 1, seed=8)[0]
    before = tables(model)
    losses, _ = model.loss_and_predictions(b)
    (losses["amm_loss_u"] + losses["amm_loss_i"]).backward()
    after = tables(model)
    moved = sorted(n for n in before if not torch.equal(before[n], after[n]))
    assert moved == ["item_tower/adgroup_id_emb", "user_tower/user_id_emb"]
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in model.dense_parameters())
    if variant == "sampled":  # only the positives' rows: the negatives' ids keep their rows
        ids = b.sparse_features["__NEG__"].values()[:16 + 12]  # (the first key: adgroup_id)
        only_negative = sorted(set(ids[16:].tolist()) - set(ids[:16].tolist()))
        assert only_negative and torch.equal(before["item_tower/adgroup_id_emb"][only_negative], after["item_tower/adgroup_id_emb"][only_negative])


@pytest.mark.parametrize("variant", VARIANTS)
def test_zero_amm_weights_move_the_tables_as_without_the_amm_call(emu, monkeypatch, variant):
    text = dv.amm_weights(dv.variant(variant), 0, 0)
    after = {}
    for skipped in (False, True):
        spec, model = build(text)
        b = dv.batches(spec, 16, 1, seed=9)[0]
        if skipped:
            monkeypatch.setattr(match, "amm_loss", lambda ua, ia, *a, **k: (ua.new_zeros(()), ua.new_zeros(())))
        (losses, _), n = counted(lambda: model.loss_and_predictions(b))
        assert n == (0 if skipped else 1) and float(losses["amm_loss_u"].detach()) == 0.0 and float(losses["amm_loss_i"].detach()) == 0.0
        sum(losses.values()).backward()
        after[skipped] = (tables(model), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    for part in (0, 1):
        assert sorted(after[False][part]) == sorted(after[True][part])
        for n in after[False][part]:
            assert torch.equal(after[False][part][n], after[True][part][n]), n


def test_evaluate_returns_recall_in_order(emu):
    from torcheasyrec_amd.metrics import Evaluator, evaluate

    for text in (dv.TEXT, dv.in_batch()):
        spec, model = build(text)
        out = evaluate(model, dv.batches(spec, 16, 3, seed=6), Evaluator(model, spec, torch.device("cpu")))
        assert sorted(out) == ["recall@1", "recall@5"] and 0.0 <= float(out["recall@1"]) <= float(out["recall@5"]) <= 1.0


SAMPLER_BLOCK = '    {kind} {{ input_path: "t" num_sample: 4 attr_fields: "adgroup_id" item_id_field: "adgroup_id" }}\n'
DATA_ANCHOR = "    num_workers: 1\n"
MODEL_ANCHOR = "    losses { softmax_cross_entropy {} }\n"
USER_TOWER = 'user_tower { input: "user" augment_input: "user_augment" mlp'
ITEM_AUGMENT = '        group_name: "item_augment"\n        feature_names: "adgroup_id"\n        group_type: DEEP\n'
REFUSALS = {
    # what every config-built match model refuses
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
    "no field 'num_towers'": (lambda t: dv.with_line(t, "        output_dim: 16\n", "        num_towers: 2\n"), ValueError),
    "user_tower has no field 'dropout'": (lambda t: t.replace(USER_TOWER, 'user_tower { input: "user" augment_input: "user_augment" dropout: 1 mlp'), ValueError),
    "similarity 'EUCLID'": (lambda t: t.replace("similarity: COSINE", "similarity: EUCLID"), ValueError),
    "needs `output_dim`": (lambda t: t.replace("        output_dim: 16\n", ""), ValueError),
    # DAT's own
    "needs `amm_i_weight`": (lambda t: t.replace("        amm_i_weight: 0.5\n", ""), ValueError),
    "needs `amm_u_weight`": (lambda t: t.replace("        amm_u_weight: 0.5\n", ""), ValueError),
    "user_tower needs `augment_input`": (lambda t: t.replace(USER_TOWER, 'user_tower { input: "user" mlp'), ValueError),
    "item_tower.augment_input 'nowhere' is not a feature group": (lambda t: t.replace('augment_input: "item_augment"', 'augment_input: "nowhere"'), ValueError),
    "item_tower.augment_input 'item_augment' is a SEQUENCE group": (lambda t: t.replace(ITEM_AUGMENT, ITEM_AUGMENT.replace("DEEP", "SEQUENCE")), ValueError),
    "user_tower.augment_input 'user_augment' is 8 wide, the towers' embedding 16": (
        lambda t: t.replace('        group_name: "user_augment"\n        feature_names: "user_id"\n', '        group_name: "user_augment"\n        feature_names: "age_level"\n'), ValueError),
    "item_tower.augment_input 'item_augment' is 16 wide, the towers' embedding 8": (lambda t: t.replace("        output_dim: 16\n", "        output_dim: 8\n").replace(
        '        group_name: "user_augment"\n        feature_names: "user_id"\n', '        group_name: "user_augment"\n        feature_names: "age_level"\n'), ValueError),
    "the towers end 16 and 12 wide": (lambda t: t.replace("        output_dim: 16\n", "        output_dim: 0\n").replace(
        'augment_input: "item_augment" mlp { hidden_units: [24, 16] }', 'augment_input: "item_augment" mlp { hidden_units: [24, 12] }'), ValueError),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refused_by_name_when_the_model_is_built(emu, name):
    make, exc = REFUSALS[name]
    text = make(dv.TEXT)
    assert text != dv.TEXT
    with pytest.raises(exc) as e:
        build(text)
    assert str(e.value).startswith("dat: ") and name in str(e.value), str(e.value)


def test_sharded_towers_are_refused(emu):
    with pytest.raises(NotImplementedError, match="process_group"):
        build(dv.TEXT, process_group=object())
