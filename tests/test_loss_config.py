"""`losses { ... }`, `num_class`, `sample_weight_fields` and the task towers' weights through the loader, the prediction keys and
the models' `loss()` (host logic and the lane emulator).  Before the block was read every model computed one plain BCE: the
tests of the other kinds fail there."""
import os

import pytest
import torch

import loss_ref as ref
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd.config import LossSpec, load_pipeline_spec
from torcheasyrec_amd.losses import session_ids
from torcheasyrec_amd.rank_model import build_rank_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BCE = "losses { binary_cross_entropy {} }"


def _text(name):
    return open(os.path.join(GOLDEN, name)).read()


def _deepfm(losses, num_class=1):
    return _text("deepfm_mini.config").replace(BCE, f"num_class: {num_class} {losses}")


def test_every_kind_parses_with_the_protos_defaults():
    spec = load_pipeline_spec(_deepfm("losses { binary_cross_entropy {} } losses { binary_focal_loss {} } losses { l2_loss {} }"))
    assert spec.losses == [LossSpec("binary_cross_entropy", {"label_smoothing": 0.0}), LossSpec("binary_focal_loss", {"gamma": 2.0, "alpha": 0.5}),
                           LossSpec("l2_loss", {})]
    spec = load_pipeline_spec(_deepfm('losses { softmax_cross_entropy {} } losses { jrc_loss { session_name: "cat_1" } }', 2))
    assert spec.losses == [LossSpec("softmax_cross_entropy", {"label_smoothing": 0.0}), LossSpec("jrc_loss", {"alpha": 0.5, "session_name": "cat_1"})]
    assert [l.name for l in spec.losses] == ["softmax_cross_entropy", "jrc_loss"] and spec.num_class == 2
    spec = load_pipeline_spec(_deepfm("losses { binary_cross_entropy { label_smoothing: 0.1 } } losses { binary_focal_loss { gamma: 1.5 alpha: 0.75 } }"))
    assert [l.fields for l in spec.losses] == [{"label_smoothing": 0.1}, {"gamma": 1.5, "alpha": 0.75}]
    assert spec.sample_weight_fields == [] and load_pipeline_spec(_text("jrc_mini.config")).sample_weight_fields == ["weight"]
    # no block: the plain BCE of before
    assert load_pipeline_spec(_text("deepfm_mini.config").replace(BCE, "")).losses == [LossSpec("binary_cross_entropy", {"label_smoothing": 0.0})]


def test_task_tower_fields_and_losses_in_tower_order():
    text = _text("mmoe_mini.config").replace(
        'label_name: "clk"', 'label_name: "clk" weight: 0.5 sample_weight_name: "w" task_space_indicator_label: "buy" in_task_space_weight: 2.0')
    spec = load_pipeline_spec(text)
    ctr, cvr = spec.task_towers
    assert (ctr.tower_name, ctr.label_name, ctr.num_class, ctr.weight, ctr.sample_weight_name, ctr.task_space_indicator_label,
            ctr.in_task_space_weight, ctr.out_task_space_weight) == ("ctr", "clk", 1, 0.5, "w", "buy", 2.0, 1.0)
    assert (cvr.weight, cvr.sample_weight_name, cvr.task_space_indicator_label, cvr.in_task_space_weight, cvr.out_task_space_weight,
            cvr.num_class) == (1.0, None, None, 1.0, 1.0, 1)
    assert [(l.name, l.tower) for l in spec.losses] == [("binary_cross_entropy_ctr", "ctr"), ("binary_cross_entropy_cvr", "cvr")]


@pytest.mark.parametrize("losses, num_class, match", [
    ("losses { binary_cross_entropy {} }", 2, "num_class must be 1"),
    ("losses { binary_focal_loss {} }", 3, "num_class must be 1"),
    ("losses { softmax_cross_entropy {} }", 1, "greater than 1"),
    ('losses { jrc_loss { session_name: "cat_1" } }', 3, "num_class must be 2"),
    ('losses { jrc_loss { session_name: "int_0" } }', 2, "not a sparse feature"),
    ('losses { jrc_loss { session_name: "nope" } }', 2, "not a sparse feature"),
    ("losses { jrc_loss {} }", 2, "session_name"),
    ("losses { binary_focal_loss { gamma: -0.5 } }", 1, "gamma"),
    ("losses { binary_focal_loss { alpha: 0.0 } }", 1, "alpha"),
    ("losses { binary_focal_loss { alpha: 1.0 } }", 1, "alpha"),
])
def test_validation_when_the_spec_is_built(losses, num_class, match):
    with pytest.raises(ValueError, match=match):
        load_pipeline_spec(_deepfm(losses, num_class))


@pytest.mark.parametrize("kind", ["recon_loss", "commitment_loss", "contrastive_loss", "hinge_loss"])
def test_sid_losses_and_unknown_kinds_are_refused_by_name(kind):
    with pytest.raises(NotImplementedError, match=f"{kind}.*binary_cross_entropy.*jrc_loss"):
        load_pipeline_spec(_deepfm(f"losses {{ {kind} {{}} }}"))


@pytest.mark.parametrize("name", ["dlrm_criteo.config", "deepfm_criteo.config", "multi_tower_din_taobao.config", "mmoe_taobao.config"])
def test_reference_configs_still_give_one_plain_bce_each(name):
    from torcheasyrec_amd.losses import build_losses

    spec = load_pipeline_spec(_text(os.path.join("reference_configs", name)))
    losses = build_losses(spec)
    assert all(l.spec.kind == "binary_cross_entropy" and l.plain_bce for l in losses)
    assert len(losses) == max(len(spec.task_towers), 1)
    assert [l.name for l in losses] == ([f"binary_cross_entropy_{t.tower_name}" for t in spec.task_towers] or ["binary_cross_entropy"])


def _first_batch(spec, B, seed=5):
    return next(iter(synthetic_batches(spec, B, B, seed=seed)))


@pytest.mark.parametrize("losses, num_class, keys", [
    ("losses { binary_cross_entropy {} }", 1, {"logits": 1, "probs": 1}),
    ("losses { binary_focal_loss {} }", 1, {"logits": 1, "probs": 1}),
    ("losses { l2_loss {} }", 1, {"y": 1}),
    ("losses { softmax_cross_entropy {} }", 3, {"logits": 2, "probs": 2}),
    ("losses { softmax_cross_entropy {} }", 2, {"logits": 2, "probs": 2, "probs1": 1}),
    ('losses { jrc_loss { session_name: "cat_1" } }', 2, {"logits": 2, "probs": 2, "probs1": 1}),
])
def test_prediction_keys_follow_the_loss_kind(dev, losses, num_class, keys):
    spec = load_pipeline_spec(_deepfm(losses, num_class))
    model = build_rank_model(spec, device=dev)
    b = _first_batch(spec, 33).to(dev)
    pred = model(b)
    assert {k: v.dim() for k, v in pred.items()} == keys
    if "probs1" in pred:
        assert torch.equal(pred["probs1"], torch.softmax(pred["logits"], dim=1)[:, 1])
    out = model.loss(pred, b)
    assert list(out) == [l.name for l in spec.losses] and all(v.dim() == 0 for v in out.values())


def _close(got, want, kind):
    import numpy as np

    gap = np.load(os.path.join(GOLDEN, "reference_loss_vectors.npz"))
    bound = 4.0 * float(gap[f"ref_gap/{kind}/loss"])
    err = abs(float(got) - float(want)) / max(1.0, abs(float(want)))
    print(f"{kind}: {float(got):.8f} against {float(want):.8f}, err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_mmoe_towers_with_focal_weights_and_a_three_class_softmax(dev):
    text = _text("mmoe_mini.config")
    text = text.replace('label_name: "clk" mlp { hidden_units: [16, 8] } losses { binary_cross_entropy {} }',
                        'label_name: "clk" mlp { hidden_units: [16, 8] } weight: 0.5 task_space_indicator_label: "buy" in_task_space_weight: 2.0 '
                        'out_task_space_weight: 0.5 losses { binary_focal_loss { gamma: 1.5 alpha: 0.75 } }')
    text = text.replace('label_name: "buy" mlp { hidden_units: [16, 8] } losses { binary_cross_entropy {} }',
                        'label_name: "buy" mlp { hidden_units: [16, 8] } num_class: 3 losses { softmax_cross_entropy { label_smoothing: 0.1 } }')
    spec = load_pipeline_spec(text)
    torch.manual_seed(11)
    model = build_rank_model(spec, device=dev)
    b = _first_batch(spec, 200).to(dev)
    pred = model(b)
    assert sorted(pred) == ["logits_ctr", "logits_cvr", "probs_ctr", "probs_cvr"] and pred["logits_cvr"].shape == (200, 3)
    out = model.loss(pred, b)
    assert list(out) == ["binary_focal_loss_ctr", "softmax_cross_entropy_cvr"]
    sum(out.values()).backward()  # one training step's backward runs through both fused gradients
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.task_outputs.parameters())
    clk, buy = b.labels["clk"].cpu(), b.labels["buy"].cpu()
    want, _ = ref.loss_and_grad("binary_focal_loss", pred["logits_ctr"].detach().cpu(), clk, gamma=1.5, alpha=0.75,
                                space_label=buy, in_w=2.0, out_w=0.5, task_weight=0.5)
    _close(out["binary_focal_loss_ctr"], want, "binary_focal_loss")
    want, _ = ref.loss_and_grad("softmax_cross_entropy", pred["logits_cvr"].detach().cpu(), buy, label_smoothing=0.1)
    _close(out["softmax_cross_entropy_cvr"], want, "softmax_cross_entropy")


def test_jrc_mini_trains_two_steps_on_its_own_logits(dev):
    spec = load_pipeline_spec(_text("jrc_mini.config"))
    assert [l.kind for l in spec.losses] == ["jrc_loss"] and spec.num_class == 2
    torch.manual_seed(12)
    model = build_rank_model(spec, device=dev)
    opt = torch.optim.SGD(list(model.dense_parameters()), lr=0.05)
    for step, hb in enumerate(synthetic_batches(spec, 2 * 96, 96, seed=6)):
        b = hb.to(dev)
        assert set(b.sample_weights) == {"weight"}
        pred = model(b)
        out = model.loss(pred, b)
        assert list(out) == ["jrc_loss"]
        want, _ = ref.loss_and_grad("jrc_loss", pred["logits"].detach().cpu(), b.labels["label"].cpu(), session_ids(b, "cat_2").cpu(),
                                    alpha=0.5, weight=b.sample_weights["weight"].cpu())
        _close(out["jrc_loss"], want, "jrc_loss")
        opt.zero_grad()
        out["jrc_loss"].backward()
        assert bool(model.output_mlp.weight.grad.abs().sum() > 0)
        opt.step()
