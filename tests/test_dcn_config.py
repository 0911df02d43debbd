"""`dcn_v1 {...}` from its config (tests/golden/dcn_mini.config): the model the reference builds from the same file
(tzrec/models/dcn.py:36-73), its cross network on csrc/cross_net.hip."""
import os

import pytest
import torch

import cross_ref as ref
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import interaction
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.interaction import Cross
from torcheasyrec_amd.metrics import Evaluator, evaluate
from torcheasyrec_amd.rank_model import ConfigDCNV1, build_rank_model

TEXT = open(os.path.join(os.path.dirname(__file__), "golden", "dcn_mini.config")).read()


def _model(dev, seed=0, text=TEXT):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    model = build_rank_model(spec, device=dev)
    with torch.no_grad():  # (the reference's zero biases would hide every bias term)
        for b in model.cross.b:
            b.copy_((0.1 * torch.randn(b.shape)).to(dev))
    return spec, model


def test_config_builds_the_references_model(dev):
    spec, model = _model(dev)
    assert spec.model_name == "dcn_v1" and type(model) is ConfigDCNV1
    assert model.embedding_group.group_total_dim("all") == 69  # four 16-wide id features + raw features of width 5: odd
    assert isinstance(model.cross, Cross) and model.cross.cross_num == 3 and model.cross.output_dim() == 69
    keys = set(model.state_dict())
    dense = {k for k in keys if not k.startswith("embedding_group.")}
    assert dense == {"cross.w.0.weight", "cross.w.1.weight", "cross.w.2.weight", "cross.b.0", "cross.b.1", "cross.b.2",
                     "deep.mlp.0.weight", "deep.mlp.0.bias", "deep.mlp.2.weight", "deep.mlp.2.bias",
                     "final_dnn.mlp.0.weight", "final_dnn.mlp.0.bias", "output_linear.weight"}
    assert "output_linear.bias" not in keys and model.output_linear.weight.shape == (1, 8)
    assert model.final_dnn.mlp[0].in_features == 69 + 16
    assert len(list(model.dense_parameters())) == len(dense)
    # cross_num defaults to 3; an unknown field of the block raises by name
    assert _model(dev, text=TEXT.replace("cross_num: 3", ""))[1].cross.cross_num == 3
    assert _model(dev, text=TEXT.replace("cross_num: 3", "cross_num: 5"))[1].cross.cross_num == 5
    with pytest.raises(ValueError, match="low_rank"):
        _model(dev, text=TEXT.replace("cross_num: 3", "cross_num: 3 low_rank: 4"))


def _recompose(features, model, dtype):
    """logits from the group's features and the model's parameters in plain torch on the CPU: the literal cross loop, the
    two MLPs (Linear + ReLU), the logits layer without bias"""
    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items() if not k.startswith("embedding_group.")}
    x = features.detach().cpu().to(dtype)
    cross = ref.cross_literal(x, [sd[f"cross.w.{i}.weight"] for i in range(3)], [sd[f"cross.b.{i}"] for i in range(3)],
                              torch.zeros_like(x), dtype)["y"][0]
    deep = x
    for i in (0, 2):
        deep = torch.relu(torch.nn.functional.linear(deep, sd[f"deep.mlp.{i}.weight"], sd[f"deep.mlp.{i}.bias"]))
    h = torch.relu(torch.nn.functional.linear(torch.cat([cross, deep], dim=-1), sd["final_dnn.mlp.0.weight"], sd["final_dnn.mlp.0.bias"]))
    return torch.nn.functional.linear(h, sd["output_linear.weight"]).squeeze(1)


def test_forward_is_the_recomposition_with_the_literal_cross(dev):
    spec, model = _model(dev, seed=1)
    batch = next(synthetic_batches(spec, 100, 100, seed=2)).to(dev)
    with torch.no_grad():
        features = model.build_input(batch)["all"]
        logits = model(batch)["logits"]
    want = _recompose(features, model, torch.float64)
    gap = ref.rel_err([_recompose(features, model, torch.float32)], [want])
    err, bound = ref.rel_err([logits], [want]), max(4.0 * gap, ref.FLOOR)
    print(f"logits on {dev.type}: err {err:.3e} gap {gap:.3e} bound {bound:.3e}")
    assert logits.shape == (100,) and err <= bound


def test_train_step_agrees_with_the_literal_twin(dev, monkeypatch):
    """one step (forward, loss, backward with the fused sparse update inside) of the fused model and of an identically seeded
    twin on the literal loop: rtol = atol = 1e-5, what tests/test_dlrm_parity.py holds a whole step to"""
    res = []
    for fused in (True, False):
        monkeypatch.setattr(interaction, "FUSED_CROSS", fused)
        spec, model = _model(dev, seed=3)
        batch = next(synthetic_batches(spec, 128, 128, seed=4)).to(dev)
        out = model(batch)
        loss = model.loss(out, batch)
        assert list(loss) == ["binary_cross_entropy"]
        loss["binary_cross_entropy"].backward()
        grads = {n: p.grad for n, p in model.named_parameters() if not n.startswith("embedding_group.")}
        assert len(grads) == 13 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()), grads.keys()
        assert all(float(grads[f"cross.{k}"].abs().max()) > 0 for k in ("w.0.weight", "w.2.weight", "b.0", "b.2"))
        tables = {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()}
        res.append((loss["binary_cross_entropy"].detach().cpu(), {n: g.detach().cpu() for n, g in grads.items()}, tables))
    (la, ga, ta), (lb, gb, tb) = res
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-5)
    for n in ga:
        torch.testing.assert_close(ga[n], gb[n], rtol=1e-5, atol=1e-5, msg=lambda m, n=n: f"{n}: {m}")
    for n in ta:
        torch.testing.assert_close(ta[n], tb[n], rtol=1e-5, atol=1e-5, msg=lambda m, n=n: f"{n}: {m}")


def test_evaluate_returns_the_configs_auc(dev):
    spec, model = _model(dev, seed=5)
    got = evaluate(model, synthetic_batches(spec, 2 * 64 + 5, 64, seed=6), Evaluator(model, spec, dev))
    assert sorted(got) == ["auc"] and 0.0 <= float(got["auc"]) <= 1.0
