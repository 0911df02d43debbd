"""`dcn_v2 {...}` from its config (tests/golden/dcn_v2_mini.config): the model the reference builds from the same file
(tzrec/models/dcn_v2.py:26-88), its low-rank cross network on csrc/cross_v2.hip."""
import os

import pytest
import torch

import cross_v2_ref as ref
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import interaction
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.interaction import CrossV2
from torcheasyrec_amd.metrics import Evaluator, evaluate
from torcheasyrec_amd.rank_model import ConfigDCNV2, build_rank_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "dcn_v2_mini.config")).read()
BACKBONE = """        backbone {
            hidden_units: [45]
        }
"""
DEEP = """        deep {
            hidden_units: [32, 16]
        }
"""
CROSS = """        cross {
            cross_num: 3
            low_rank: 8
        }
"""
FINAL = """        final {
            hidden_units: [8]
        }
"""
CROSS_KEYS = {f"cross.u_kernels.{i}.weight" for i in range(3)} | {f"cross.v_kernels.{i}.{n}" for i in range(3) for n in ("weight", "bias")}
DEEP_KEYS = {"deep.mlp.0.weight", "deep.mlp.0.bias", "deep.mlp.2.weight", "deep.mlp.2.bias"}
BACKBONE_KEYS = {"backbone.mlp.0.weight", "backbone.mlp.0.bias"}
TAIL_KEYS = {"final_dnn.mlp.0.weight", "final_dnn.mlp.0.bias", "output_linear.weight"}


def _model(dev, seed=0, text=TEXT):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=dev)


def _dense_keys(model):
    return {k for k in model.state_dict() if not k.startswith("embedding_group.")}


def test_the_blocks_are_in_the_text():
    assert all(TEXT.count(b) == 1 for b in (BACKBONE, DEEP, CROSS, FINAL))


def test_config_builds_the_references_model(dev):
    spec, model = _model(dev)
    assert spec.model_name == "dcn_v2" and type(model) is ConfigDCNV2
    assert model.embedding_group.group_total_dim("all") == 69  # four 16-wide id features + raw features of width 5: odd
    assert isinstance(model.cross, CrossV2) and model.cross.cross_num == 3 and model.cross._low_rank == 8
    assert _dense_keys(model) == CROSS_KEYS | DEEP_KEYS | BACKBONE_KEYS | TAIL_KEYS
    assert "output_linear.bias" not in model.state_dict() and model.output_linear.weight.shape == (1, 8)
    # `cross` reads the backbone's output, `deep` the group, `final_dnn` cross + deep
    assert model.backbone.mlp[0].in_features == 69 and model.cross.output_dim() == 45
    assert model.cross.u_kernels[0].weight.shape == (8, 45) and model.cross.v_kernels[2].weight.shape == (45, 8)
    assert model.deep.mlp[0].in_features == 69 and model.final_dnn.mlp[0].in_features == 45 + 16
    assert len(list(model.dense_parameters())) == len(_dense_keys(model))


@pytest.mark.parametrize("backbone", [True, False])
@pytest.mark.parametrize("deep", [True, False])
def test_backbone_and_deep_are_optional(dev, backbone, deep):
    text = TEXT if backbone else TEXT.replace(BACKBONE, "")
    text = text if deep else text.replace(DEEP, "")
    spec, model = _model(dev, text=text)
    assert (model.backbone is not None) == backbone and (model.deep is not None) == deep
    assert _dense_keys(model) == CROSS_KEYS | TAIL_KEYS | (BACKBONE_KEYS if backbone else set()) | (DEEP_KEYS if deep else set())
    d_cross = 45 if backbone else 69
    assert model.cross.output_dim() == d_cross and model.final_dnn.mlp[0].in_features == d_cross + (16 if deep else 0)
    batch = next(synthetic_batches(spec, 20, 20, seed=2)).to(dev)
    out = model(batch)
    loss = model.loss(out, batch)["binary_cross_entropy"]
    loss.backward()
    assert out["logits"].shape == (20,) and bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.dense_parameters())


def test_defaults_unknown_fields_and_missing_blocks(dev):
    m = _model(dev, text=TEXT.replace("cross_num: 3", "").replace("low_rank: 8", ""))[1]
    assert m.cross.cross_num == 3 and m.cross._low_rank == 32 and m.cross.u_kernels[0].weight.shape == (32, 45)
    m = _model(dev, text=TEXT.replace("cross_num: 3", "cross_num: 5").replace("low_rank: 8", "low_rank: 3"))[1]
    assert m.cross.cross_num == 5 and m.cross._low_rank == 3
    with pytest.raises(ValueError, match="cin_layer_size"):
        _model(dev, text=TEXT.replace("low_rank: 8", "low_rank: 8 cin_layer_size: 4"))
    with pytest.raises(ValueError, match="wide"):
        _model(dev, text=TEXT.replace(FINAL, FINAL + "        wide { hidden_units: [4] }\n"))
    with pytest.raises(ValueError, match="cross"):
        _model(dev, text=TEXT.replace(CROSS, ""))
    with pytest.raises(ValueError, match="final"):
        _model(dev, text=TEXT.replace(FINAL, ""))
    # dcn_v1 keeps refusing low_rank
    v1 = open(os.path.join(GOLDEN, "dcn_mini.config")).read()
    with pytest.raises(ValueError, match="low_rank"):
        _model(dev, text=v1.replace("cross_num: 3", "cross_num: 3 low_rank: 4"))


def _recompose(features, model, dtype):
    """logits from the group's features and the model's parameters in plain torch on the CPU: the backbone, the literal cross
    loop over its output, the deep MLP over the features (Linear + ReLU), the final MLP, the logits layer without bias"""
    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items() if not k.startswith("embedding_group.")}
    lin = torch.nn.functional.linear
    x = features.detach().cpu().to(dtype)
    net = torch.relu(lin(x, sd["backbone.mlp.0.weight"], sd["backbone.mlp.0.bias"]))
    cross = ref.literal(net, [sd[f"cross.u_kernels.{i}.weight"] for i in range(3)], [sd[f"cross.v_kernels.{i}.weight"] for i in range(3)],
                        [sd[f"cross.v_kernels.{i}.bias"] for i in range(3)], torch.zeros_like(net), dtype)["y"][0]
    deep = x
    for i in (0, 2):
        deep = torch.relu(lin(deep, sd[f"deep.mlp.{i}.weight"], sd[f"deep.mlp.{i}.bias"]))
    h = torch.relu(lin(torch.cat([cross, deep], dim=-1), sd["final_dnn.mlp.0.weight"], sd["final_dnn.mlp.0.bias"]))
    return lin(h, sd["output_linear.weight"]).squeeze(1)


def test_forward_is_the_recomposition_with_the_literal_cross(dev, monkeypatch):
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", True)
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
    twin on the literal loop: rtol = atol = 1e-5, what tests/test_dcn_config.py holds the v1 step to"""
    res = []
    for fused in (True, False):
        monkeypatch.setattr(interaction, "FUSED_CROSS_V2", fused)
        spec, model = _model(dev, seed=3)
        batch = next(synthetic_batches(spec, 128, 128, seed=4)).to(dev)
        out = model(batch)
        loss = model.loss(out, batch)
        assert list(loss) == ["binary_cross_entropy"]
        loss["binary_cross_entropy"].backward()
        grads = {n: p.grad for n, p in model.named_parameters() if not n.startswith("embedding_group.")}
        assert len(grads) == 18 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()), grads.keys()
        assert all(float(grads[k].abs().max()) > 0 for k in CROSS_KEYS)
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
