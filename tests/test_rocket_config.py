"""`rocket_launching {...}` from its config (tests/golden/rocket_mini.config and its variants, tests/rocket_variants.py): the model
the reference builds from the same file (tzrec/models/rocket_launching.py:38-245) -- its prediction and loss keys in training and
in evaluation, the layer pairing, where each loss's gradient goes and where it does not, the fused distillation terms called once a
training step and never in evaluation, the flag-off behaviour, the refusals, and the evaluator's `auc_light`."""
import pytest
import torch

import rocket_variants as rv
from mlp_ref import FLOOR, rel_err
from torcheasyrec_amd import _lib, rocket
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.metrics import Evaluator, evaluate
from torcheasyrec_amd.rank_model import _MODELS, build_rank_model

# the model block of the reference's examples/rocket_launching_criteo.config (no share MLP, the default COSINE function)
CRITEO_BLOCK = """    rocket_launching {
        booster_mlp {
            hidden_units: [256, 128, 64, 32]
        }
        light_mlp {
            hidden_units: [96, 64, 32]
        }
        feature_based_distillation: true
    }
"""


def build(text, dev, seed=0):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=dev)


def counted(fn):
    calls, L = [], _lib.lib()
    orig = L.tzr_distill_loss_fwd
    L.tzr_distill_loss_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        return fn(), len(calls)
    finally:
        L.tzr_distill_loss_fwd = orig


def dense_keys(model):
    return sorted(k for k in model.state_dict() if not k.startswith("embedding_group."))


def mlp_keys(name, n):
    return [f"{name}.mlp.{2 * i}.{p}" for i in range(n) for p in ("weight", "bias")]


def tables(model):
    return {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()}


def expected_keys(name, training):
    two = name == "two_class"
    sides = ["_booster", "_light"] if training else ["_light"]
    preds = [k + s for s in sides for k in (("logits", "probs", "probs1") if two else ("logits", "probs"))]
    kind = "softmax_cross_entropy" if two else "binary_cross_entropy"
    losses = [kind + s for s in sides]
    if training:
        losses.append("hint_l2_loss")
        if name != "flag_off":
            preds += ["light_0", "light_1", "booster_1", "booster_2"]
            losses += ["similarity_0_1", "similarity_1_2"]
    return sorted(preds), sorted(losses)


@pytest.mark.parametrize("name", rv.NAMES)
def test_every_variant_builds_and_has_the_references_keys(dev, name):
    spec, model = build(rv.variant(name), dev)
    assert spec.model_name == "rocket_launching" and type(model) is _MODELS["rocket_launching"] is rocket.ConfigRocketLaunching
    # the reference's parameter names, its MLP's `mlp.<i>.perceptron.0` being this package's `mlp.<2i>`
    want = mlp_keys("booster_mlp", 3) + mlp_keys("light_mlp", 2) + [f"{l}.{p}" for l in ("booster_linear", "light_linear") for p in ("weight", "bias")]
    want += mlp_keys("share_mlp", 1) if name != "no_share" else []
    assert dense_keys(model) == sorted(want) and (model.share_mlp is None) == (name == "no_share")
    C = 2 if name == "two_class" else 1
    assert model.booster_linear.weight.shape == (C, 8) and model.light_linear.weight.shape == (C, 8)
    assert model.booster_mlp.mlp[0].in_features == model.light_mlp.mlp[0].in_features == (69 if name == "no_share" else 24)
    assert model.mlp_index_dict == {0: 1, 1: 2}  # light [16, 8] against booster [32, 16, 8]
    assert model._cosine == (name != "distance")
    b = rv.batches(spec, 9, 1)[0].to(dev)
    pred_keys, loss_keys = expected_keys(name, True)
    out = model(b)
    (losses, n) = counted(lambda: model.loss(out, b))
    assert sorted(out) == pred_keys and sorted(losses) == loss_keys and n == 1
    assert out["logits_light"].shape == ((9, 2) if C == 2 else (9,))
    assert all(l.dim() == 0 and bool(torch.isfinite(l)) for l in losses.values())
    model.eval()
    with torch.no_grad():
        out = model(b)
        (losses, n) = counted(lambda: model.loss(out, b))
    pred_keys, loss_keys = expected_keys(name, False)
    assert sorted(out) == pred_keys and sorted(losses) == loss_keys and n == 0  # no booster key, no distillation term, no kernel


def test_the_booster_does_not_run_in_evaluation(dev):
    spec, model = build(rv.variant("mini"), dev)
    ran = []
    model.booster_mlp.register_forward_hook(lambda *a: ran.append("mlp"))
    model.booster_linear.register_forward_hook(lambda *a: ran.append("linear"))
    b = rv.batches(spec, 9, 1)[0].to(dev)
    model(b)
    assert ran == ["mlp", "linear"]
    model.eval()
    with torch.no_grad():
        model(b)
    assert ran == ["mlp", "linear"]


def test_the_criteo_examples_model_block_builds_and_pairs_its_layers(dev):
    text = rv.swap(rv.variant("two_class"), rv.TEXT[rv.TEXT.index("    rocket_launching {"):rv.TEXT.index("    num_class: 1\n")], CRITEO_BLOCK)
    spec, model = build(text, dev)
    assert model.share_mlp is None and model._cosine and model._feature_based and spec.num_class == 2
    assert model.booster_mlp.hidden_units == [256, 128, 64, 32] and model.light_mlp.hidden_units == [96, 64, 32]
    assert model.mlp_index_dict == {1: 2, 2: 3}
    b = rv.batches(spec, 9, 1)[0].to(dev)
    out = model(b)
    losses, n = counted(lambda: model.loss(out, b))
    assert n == 1 and sorted(losses) == ["hint_l2_loss", "similarity_1_2", "similarity_2_3", "softmax_cross_entropy_booster", "softmax_cross_entropy_light"]
    assert out["light_1"].shape == out["booster_2"].shape == (9, 64) and out["light_2"].shape == out["booster_3"].shape == (9, 32)


def grads_of(model, loss):
    for p in model.parameters():
        p.grad = None
    loss.backward()
    return {n: p.grad for n, p in model.named_parameters() if not n.startswith("embedding_group.")}


@pytest.mark.parametrize("name", ["mini", "two_class", "distance"])
def test_where_each_losss_gradient_goes(dev, name):
    """the light net reads share_net.detach() and every booster operand of the distillation terms is detached: the light side's
    losses reach the light net alone -- the tables (updated inside the backward) stay bit for bit, the share MLP and the booster
    get nothing --, the booster's own loss reaches the booster, the share MLP and the tables and nothing of the light net"""
    kind = "softmax_cross_entropy" if name == "two_class" else "binary_cross_entropy"
    # (a) the light side: its classification loss, the hint and both similarity terms
    spec, model = build(rv.variant(name), dev, seed=3)
    b = rv.batches(spec, 16, 1, seed=4)[0].to(dev)
    before = tables(model)
    losses = model.loss(model(b), b)
    g = grads_of(model, sum(v for k, v in losses.items() if k != kind + "_booster"))
    after = tables(model)
    assert all(torch.equal(before[n], after[n]) for n in before)
    for n, d in g.items():
        if n.startswith("light_"):
            assert d is not None and bool(torch.isfinite(d).all()) and float(d.abs().max()) > 0, n
        else:
            assert d is None or float(d.abs().max()) == 0.0, n
    # (b) the hint and the similarity terms alone: nothing for the booster, and they do move the light net
    spec, model = build(rv.variant(name), dev, seed=3)
    losses = model.loss(model(b), b)
    g = grads_of(model, sum(v for k, v in losses.items() if not k.startswith(kind)))
    assert all(d is None or float(d.abs().max()) == 0.0 for n, d in g.items() if not n.startswith("light_"))
    assert all(float(g[f"light_mlp.mlp.{i}.weight"].abs().max()) > 0 for i in (0, 2)) and float(g["light_linear.weight"].abs().max()) > 0
    # (c) the booster's classification loss
    spec, model = build(rv.variant(name), dev, seed=3)
    before = tables(model)
    losses = model.loss(model(b), b)
    g = grads_of(model, losses[kind + "_booster"])
    after = tables(model)
    assert any(not torch.equal(before[n], after[n]) for n in before)
    for n, d in g.items():
        if n.startswith("light_"):
            assert d is None or float(d.abs().max()) == 0.0, n
        else:
            assert d is not None and float(d.abs().max()) > 0, n


@pytest.mark.parametrize("name", ["mini", "no_weights", "two_class", "distance", "flag_off"])
def test_the_fused_terms_are_the_literal_ones(dev, monkeypatch, name):
    """one training step under FUSED_DISTILL_LOSS True and False: every loss and every dense gradient within max(4 x gap, 2^-20)
    of a float64 evaluation of the distillation terms on the fused run's own predictions, gap the fp32 literal form's distance"""
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(rocket, "FUSED_DISTILL_LOSS", fused)
        spec, model = build(rv.variant(name), dev, seed=5)
        b = rv.batches(spec, 16, 1, seed=6)[0].to(dev)
        out = model(b)
        losses, n = counted(lambda: model.loss(out, b))
        assert n == (1 if fused else 0)
        g = grads_of(model, sum(losses.values()))
        res[fused] = ({k: v.detach().cpu() for k, v in losses.items()}, {k: v.detach().cpu() for k, v in g.items() if v is not None}, out)
    (la, ga, out), (lb, gb, _) = res[True], res[False]
    assert sorted(la) == sorted(lb) and sorted(ga) == sorted(gb)
    w = b.sample_weights["weight"].double().cpu() if spec.sample_weight_fields else None
    pairs = model._pairs
    sims64, hint64 = rocket.distill_losses_literal([out[f"light_{i}"].detach().double().cpu() for i, _ in pairs],
                                                   [out[f"booster_{j}"].detach().double().cpu() for _, j in pairs],
                                                   out["logits_light"].detach().double().cpu(), out["logits_booster"].detach().double().cpu(), model._cosine, w)
    names = [f"similarity_{i}_{j}" for i, j in pairs] + ["hint_l2_loss"]
    want = [t for t in sims64 + (hint64,)]
    gap = rel_err([lb[k] for k in names], want)
    err = rel_err([la[k] for k in names], want)
    print(f"{name} on {dev.type}: distillation terms err {err:.3e} gap {gap:.3e}")
    assert err <= max(4.0 * gap, FLOOR)
    for k in la:
        torch.testing.assert_close(la[k], lb[k], rtol=1e-5, atol=1e-6, msg=lambda m, k=k: f"{k}: {m}")
    for k in ga:
        torch.testing.assert_close(ga[k], gb[k], rtol=1e-4, atol=1e-6, msg=lambda m, k=k: f"{k}: {m}")


def test_with_the_flag_off_the_hint_loss_alone_is_added(dev):
    """a deliberate difference (NOTES.md): the reference's training forward raises here -- it indexes the MLP's output tensor by
    "hidden_layer<i>" whenever two widths agree -- ; this model publishes no hidden layer and adds the hint loss alone"""
    spec, model = build(rv.variant("flag_off"), dev)
    assert not model._feature_based and model.mlp_index_dict == {0: 1, 1: 2} and model._pairs == []
    assert not model.booster_mlp.return_hidden_layer_feature and not model.light_mlp.return_hidden_layer_feature
    b = rv.batches(spec, 9, 1)[0].to(dev)
    out = model(b)
    losses, n = counted(lambda: model.loss(out, b))
    assert n == 1 and sorted(losses) == ["binary_cross_entropy_booster", "binary_cross_entropy_light", "hint_l2_loss"]
    assert not any(k.startswith(("light_", "booster_")) for k in out)
    w = b.sample_weights["weight"].double().cpu()
    lw = w / w.mean()
    want = ((out["logits_light"].detach().double().cpu() - out["logits_booster"].detach().double().cpu()) ** 2 * lw).mean()
    assert abs(float(losses["hint_l2_loss"].detach()) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))


def test_refusals_by_name(dev):
    with pytest.raises(ValueError, match="booster_mlp"):
        build(rv.swap(rv.TEXT, rv.BOOSTER, ""), dev)
    with pytest.raises(ValueError, match="light_mlp"):
        build(rv.swap(rv.TEXT, rv.LIGHT, ""), dev)
    two = rv.swap(rv.swap(rv.TEXT, rv.CLASSES, "    num_class: 2\n"), rv.LOSSES, "    losses { softmax_cross_entropy {} }\n")
    with pytest.raises(ValueError, match="sample weights.*num_class 2"):
        build(two, dev)
    with pytest.raises(ValueError, match="final"):
        build(rv.swap(rv.TEXT, rv.FLAG, rv.FLAG + "        final { hidden_units: [4] }\n"), dev)


@pytest.mark.parametrize("name", ["mini", "two_class"])
def test_the_evaluator_keys_auc_light(dev, name):
    spec, model = build(rv.variant(name), dev, seed=7)
    assert model.metric_suffixes() == ["_light"]
    ev = Evaluator(model, spec, dev)
    assert sorted(ev.metrics) == ["auc_light"] and ev._probs_key == {"_light": "probs1_light" if name == "two_class" else "probs_light"}
    got, n = counted(lambda: evaluate(model, rv.batches(spec, 64, 2, seed=8), ev))
    assert n == 0 and sorted(got) == ["auc_light"] and 0.0 <= float(got["auc_light"]) <= 1.0 and model.training
    # the metric read the light net's probabilities
    from torcheasyrec_amd.metrics import BinnedAUC

    auc = BinnedAUC(200, device=dev)
    model.eval()
    with torch.no_grad():
        for hb in rv.batches(spec, 64, 2, seed=8):
            b = hb.to(dev)
            p = model(b)["probs1_light" if name == "two_class" else "probs_light"]
            auc.update(p, b.labels["label"])
    assert float(auc.compute()) == float(got["auc_light"])


def test_an_existing_configs_evaluator_is_unchanged(dev):
    import os

    golden = os.path.join(os.path.dirname(__file__), "golden")
    spec, model = build(open(os.path.join(golden, "dcn_v2_mini.config")).read(), dev)
    assert not hasattr(model, "metric_suffixes")
    ev = Evaluator(model, spec, dev)
    assert sorted(ev.metrics) == ["auc"] and ev._probs_key == {"": "probs"} and ev._towers == {"": ["auc"]}
    spec, model = build(open(os.path.join(golden, "ple_mini.config")).read(), dev)
    ev = Evaluator(model, spec, dev)
    assert sorted(ev.metrics) == sorted(ms.name for ms in spec.metrics) and all(k for k in ev._towers)  # per tower, as before
    assert ev._probs_key == {s: "probs" + s for s in ev._towers}
