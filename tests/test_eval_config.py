"""`model_config.metrics` through the loader, the Evaluator and `evaluate()` (host logic and the lane emulator)."""
import os

import pytest
import torch

import metrics_ref as ref
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import _lib
from torcheasyrec_amd.config import MetricSpec, load_pipeline_spec
from torcheasyrec_amd.metrics import Evaluator, evaluate, first_id_per_sample
from torcheasyrec_amd.rank_model import build_rank_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MORE = 'metrics { auc {} } metrics { grouped_auc { grouping_key: "cat_1" } } metrics { normalized_entropy {} }'


def _text(name):
    return open(os.path.join(GOLDEN, name)).read()


@pytest.mark.parametrize("name", ["deepfm_mini.config", "din_mini.config"])
def test_shipped_configs_yield_one_auc_spec(name):
    spec = load_pipeline_spec(_text(name))
    assert spec.metrics == [MetricSpec(kind="auc", fields={"thresholds": 200}, tower=None, label=spec.label_fields[0])]
    assert spec.metrics[0].name == "auc" and spec.metrics[0].suffix == ""


def test_grouped_auc_and_normalized_entropy_are_parsed():
    spec = load_pipeline_spec(_text("deepfm_mini.config").replace("metrics { auc {} }", MORE.replace("auc {}", "auc { thresholds: 50 }")))
    assert [(m.kind, m.fields) for m in spec.metrics] == [("auc", {"thresholds": 50}), ("grouped_auc", {"grouping_key": "cat_1"}),
                                                          ("normalized_entropy", {"eta": 1e-12})]
    with pytest.raises(ValueError, match="grouping_key"):
        load_pipeline_spec(_text("deepfm_mini.config").replace("metrics { auc {} }", "metrics { grouped_auc {} }"))
    # a kind that is read but not built loads all the same, its fields as written
    spec = load_pipeline_spec(_text("deepfm_mini.config").replace("metrics { auc {} }", "metrics { accuracy { threshold: 0.25 } } metrics { xauc {} }"))
    assert [(m.kind, m.fields) for m in spec.metrics] == [("accuracy", {"threshold": 0.25, "top_k": 1}), ("xauc", {"sample_ratio": 1e-3, "in_batch": False})]
    assert load_pipeline_spec(_text("mmoe_mini.config")).metrics == []


def test_task_tower_metrics_carry_the_tower_suffix():
    text = _text("mmoe_mini.config").replace('label_name: "clk"', 'label_name: "clk" metrics { auc {} } metrics { normalized_entropy { eta: 1e-6 } }')
    text = text.replace('label_name: "buy"', 'label_name: "buy" metrics { auc { thresholds: 100 } }')
    spec = load_pipeline_spec(text)
    assert [(m.name, m.tower, m.label, m.fields) for m in spec.metrics] == [
        ("auc_ctr", "ctr", "clk", {"thresholds": 200}), ("normalized_entropy_ctr", "ctr", "clk", {"eta": 1e-6}),
        ("auc_cvr", "cvr", "buy", {"thresholds": 100})]


def test_unbuilt_kind_raises_in_the_evaluator_by_name(dev):
    spec = load_pipeline_spec(_text("deepfm_mini.config").replace("metrics { auc {} }", "metrics { auc {} } metrics { accuracy {} }"))
    model = build_rank_model(spec, device=dev)
    with pytest.raises(NotImplementedError, match="accuracy"):
        Evaluator(model, spec, dev)


def test_package_exports():
    import torcheasyrec_amd as pkg
    from torcheasyrec_amd import metrics

    for name in ("BinnedAUC", "GroupedAUC", "NormalizedEntropy", "Evaluator", "evaluate"):
        assert getattr(pkg, name) is getattr(metrics, name)


def test_first_id_per_sample_is_the_first_id_or_zero():
    from torcheasyrec_amd.sparse import KeyedJaggedTensor

    jag = KeyedJaggedTensor(["a", "b"], torch.tensor([5, 6, 7, 8, 9]), torch.tensor([2, 0, 1, 1, 0, 1], dtype=torch.int32))
    assert first_id_per_sample(jag, "a").tolist() == [5, 0, 7] and first_id_per_sample(jag, "b").tolist() == [8, 0, 9]
    uni = KeyedJaggedTensor(["a", "b"], torch.tensor([1, 2, 3, 4]), torch.ones(4, dtype=torch.int32), uniform_length=1)
    assert first_id_per_sample(uni, "b").tolist() == [3, 4]


def test_evaluate_computes_the_configs_metrics_and_moves_no_parameter(dev):
    spec = load_pipeline_spec(_text("deepfm_mini.config").replace("metrics { auc {} }", MORE))
    torch.manual_seed(3)
    model = build_rank_model(spec, device=dev)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    before.update({f"table:{n}": w.detach().clone() for n, w in model.embedding_group.ebc.table_weights().items()})
    before.update({f"state:{n}": w.detach().clone() for n, w in model.embedding_group.ebc.table_states().items()})
    batches = list(synthetic_batches(spec, 3 * 64 + 5, 64, seed=4))  # three full batches and a short one
    ev = Evaluator(model, spec, dev)
    assert model.training
    got = evaluate(model, batches, ev)
    assert model.training and sorted(got) == ["auc", "grouped_auc", "normalized_entropy"]
    after = {n: p.detach() for n, p in model.named_parameters()}
    after.update({f"table:{n}": w.detach() for n, w in model.embedding_group.ebc.table_weights().items()})
    after.update({f"state:{n}": w.detach() for n, w in model.embedding_group.ebc.table_states().items()})
    assert before.keys() == after.keys() and all(torch.equal(before[n], after[n]) for n in before), "evaluate() moved a parameter"
    # the same predictions through the restatement
    model.eval()
    with torch.no_grad():
        probs = torch.cat([model(b.to(dev))["probs"].cpu() for b in batches])
    model.train()
    labels = torch.cat([b.labels["label"] for b in batches])
    keys = torch.cat([first_id_per_sample(b.sparse_features["__BASE__"], "cat_1") for b in batches])
    thr = ev.metrics["auc"].thresholds.cpu()
    assert torch.equal(ev.metrics["auc"].confmat().cpu(), ref.confmat(probs, labels, thr))
    torch.testing.assert_close(got["auc"].cpu(), ref.auc_from_confmat(ref.confmat(probs, labels, thr)), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(got["grouped_auc"].cpu(), torch.tensor(ref.grouped_auc(probs, labels, keys), dtype=torch.float64), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(got["normalized_entropy"].cpu().to(torch.float64), ref.normalized_entropy(probs, labels), rtol=1e-5, atol=0.0)
    ev.reset()
    assert int(ev.metrics["auc"].histogram().sum()) == 0 and ev.metrics["grouped_auc"].rows()[3] == 0


def test_evaluate_multi_task_towers(dev):
    text = _text("mmoe_mini.config").replace('label_name: "clk"', 'label_name: "clk" metrics { auc {} }')
    text = text.replace('label_name: "buy"', 'label_name: "buy" metrics { auc {} } metrics { normalized_entropy {} }')
    text = text.replace("zch { zch_size: 128 eviction_interval: 2 lfu {} }", "num_buckets: 128")
    spec = load_pipeline_spec(text)
    torch.manual_seed(5)
    model = build_rank_model(spec, device=dev)
    batches = list(synthetic_batches(spec, 100, 50, seed=6))
    ev = Evaluator(model, spec, dev)
    got = evaluate(model, batches, ev)
    assert sorted(got) == ["auc_ctr", "auc_cvr", "normalized_entropy_cvr"]
    model.eval()
    with torch.no_grad():
        preds = [model(b.to(dev)) for b in batches]
    for tower, label in (("ctr", "clk"), ("cvr", "buy")):
        probs = torch.cat([p[f"probs_{tower}"].cpu() for p in preds])
        labels = torch.cat([b.labels[label] for b in batches])
        assert torch.equal(ev.metrics[f"auc_{tower}"].confmat().cpu(), ref.confmat(probs, labels, torch.linspace(0, 1, 200)))
