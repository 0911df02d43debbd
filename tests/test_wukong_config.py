"""`wukong {...}` from its config (tests/golden/wukong_mini.config): the model the reference builds from the same file
(tzrec/models/wukong.py:36-130), each layer's FM front and mix on csrc/wukong.hip."""
import itertools
import os

import pytest
import torch

from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import _lib
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.dense_optim import build_dense_optimizer, named_dense_parameters
from torcheasyrec_amd.embedding_group import TrainPipeline
from torcheasyrec_amd.optimizer import build_train_optimizer
from torcheasyrec_amd.rank_model import ConfigWuKong, build_rank_model
from torcheasyrec_amd.wukong import LinearCompressBlock, WuKongLayer

TEXT = open(os.path.join(os.path.dirname(__file__), "golden", "wukong_mini.config")).read()
DENSE_GROUP = TEXT[TEXT.index("    feature_groups {\n        group_name: \"dense\""):TEXT.index("    feature_groups {\n        group_name: \"sparse\"")]
SEQ_FEATURE = ("feature_configs { sequence_feature { sequence_name: \"click_seq\" sequence_length: 8 sequence_delim: \"|\"\n"
               "    features { id_feature { feature_name: \"cat_0\" num_buckets: 1000 embedding_dim: 8 } } } }\nmodel_config {")
SEQ_GROUP = ("        sequence_groups { group_name: \"click_seq\" feature_names: \"cat_0\" feature_names: \"click_seq__cat_0\" }\n"
             "        sequence_encoders { pooling_encoder { pooling_type: \"mean\" } }\n        group_type: DEEP")


def _model(dev, seed=0, text=TEXT):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=dev)


def _layer_keys(i, projection):
    keys = ["lcb.weight", "fmb.weight", "fmb.norm.weight", "fmb.norm.bias", "fmb.mlp.mlp.0.weight", "fmb.mlp.mlp.0.bias",
            "fmb.feature_out_liner.weight", "fmb.feature_out_liner.bias", "norm.weight", "norm.bias"]
    return {f"_wukong_layers.{i}.{k}" for k in keys + (["residual_projection.weight"] if projection else [])}


def test_config_builds_the_references_model(dev):
    spec, model = _model(dev)
    assert spec.model_name == "wukong" and type(model) is ConfigWuKong
    eg = model.embedding_group
    assert eg.group_total_dim("dense") == 5 and eg.group_dims("sparse") == [8] * 4
    l0, l1 = model._wukong_layers
    assert isinstance(l0, WuKongLayer) and isinstance(l0.residual_projection, LinearCompressBlock) and isinstance(l1.residual_projection, torch.nn.Identity)
    assert (l0.fmb.feature_num_in, l0.fmb_feature_num, l0.lcb_feature_num, l0.fmb.compressed_feature_num) == (5, 4, 3, 3)
    assert (l1.fmb.feature_num_in, l1.fmb_feature_num, l1.lcb_feature_num, l1.fmb.compressed_feature_num) == (7, 3, 4, 3)
    assert l0.output_feature_num() == 7 and l1.output_feature_num() == 7
    # the reference's parameter names (its MLP's Linear of layer i is `mlp.<i>.perceptron.0`, this package's `mlp.<2i>`)
    dense = {k for k in model.state_dict() if not k.startswith("embedding_group.")}
    assert dense == _layer_keys(0, True) | _layer_keys(1, False) \
        | {f"{m}.mlp.{i}.{w}" for m in ("dense_mlp", "final_mlp") for i in (0, 2) for w in ("weight", "bias")} | {"output_mlp.weight", "output_mlp.bias"}
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert shapes["_wukong_layers.0.lcb.weight"] == (5, 3) and shapes["_wukong_layers.0.residual_projection.weight"] == (5, 7)
    assert shapes["_wukong_layers.0.fmb.weight"] == (5, 3) and shapes["_wukong_layers.0.fmb.norm.weight"] == (15,)
    assert shapes["_wukong_layers.0.fmb.mlp.mlp.0.weight"] == (12, 15) and shapes["_wukong_layers.0.fmb.feature_out_liner.weight"] == (32, 12)
    assert shapes["_wukong_layers.1.fmb.weight"] == (7, 3) and shapes["_wukong_layers.1.fmb.feature_out_liner.weight"] == (24, 12)
    assert shapes["_wukong_layers.1.norm.weight"] == (8,) and shapes["final_mlp.mlp.0.weight"] == (8, 56) and shapes["output_mlp.weight"] == (1, 4)
    # kaiming_uniform_ on the two kinds of weight: |w| <= sqrt(6 / fan_in), fan_in = the second extent
    for k, bound in (("_wukong_layers.0.lcb.weight", (6 / 3) ** 0.5), ("_wukong_layers.1.fmb.weight", (6 / 3) ** 0.5)):
        w = model.state_dict()[k]
        assert 0.3 * bound < float(w.abs().max()) <= bound


def test_the_single_group_form_and_the_default_k(dev):
    """one group: it is the sparse one whatever its name, and there is no dense row; compressed_feature_num defaults to 16"""
    text = TEXT.replace(DENSE_GROUP, "").replace('group_name: "sparse"', 'group_name: "all"').replace("        dense_mlp {\n            hidden_units: [16, 8]\n        }\n", "")
    text = text.replace("compressed_feature_num: 3", "", 1)
    assert 'group_name: "dense"' not in text and "dense_mlp" not in text and text.count("compressed_feature_num") == 1
    spec, model = _model(dev, text=text)
    l0, l1 = model._wukong_layers
    assert model.dense_mlp is None and l0.fmb.feature_num_in == 4 and l0.fmb.compressed_feature_num == 16 and l1.fmb.compressed_feature_num == 3
    assert tuple(l0.fmb.weight.shape) == (4, 16) and l0.fmb.norm.normalized_shape == (64,)
    batch = next(synthetic_batches(spec, 9, 9, seed=2)).to(dev)
    out = model(batch)
    assert out["logits"].shape == (9,) and bool(torch.isfinite(out["logits"]).all())


def _count_calls():
    lib, n = _lib.lib(), [0, 0]
    names = ("tzr_wukong_fm_fwd", "tzr_wukong_mix_fwd", "tzr_wukong_fm_bwd", "tzr_wukong_mix_bwd")
    orig = {nm: getattr(lib, nm) for nm in names}

    def counted(nm, slot):
        def f(*a):
            n[slot] += 1
            return orig[nm](*a)
        return f

    for i, nm in enumerate(names):
        setattr(lib, nm, counted(nm, i // 2))

    def done():
        for nm in names:
            setattr(lib, nm, orig[nm])
        return tuple(n)

    return done


def test_twenty_steps_bring_the_loss_down(dev):
    """the loop of examples/train_from_config.py (forward, backward, the fused dense optimizer's step) over one batch of
    synthetic_batches seen 20 times: finite losses under the config's loss name that go down; two layers x 2 entry points each way
    per step.  (Which parameters get a non-zero gradient is not asked here: with `final [8, 4]` and 16 samples a draw can leave the
    last ReLU layer dead, and then only the logits layer's bias learns; every gradient of a layer is held to the reference in
    tests/test_wukong_module.py.)"""
    spec, model = _model(dev, seed=3)
    opt = build_dense_optimizer(named_dense_parameters(model), spec.dense_optimizer)
    pipe = TrainPipeline(model, build_train_optimizer(opt, spec.grad_clipping, spec.gradient_accumulation_steps), dev, model.loss)
    batch = next(synthetic_batches(spec, 16, 16, seed=4))  # (16 samples: the emulator runs a workgroup of fibers per sample and launch)
    it, losses = itertools.repeat(batch, 20), []
    calls = _count_calls()
    try:
        for _ in range(20):
            l, _, _ = pipe.progress(it)
            assert list(l) == ["binary_cross_entropy"]
            losses.append(float(l["binary_cross_entropy"].detach()))
    finally:
        n = calls()
    print(f"losses on {dev.type}: {losses}")
    assert n == (80, 80)
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0] and sum(losses[-5:]) < sum(losses[:5]), losses


@pytest.mark.parametrize("text,message", [
    (TEXT.replace('"cat_1" num_buckets: 3 embedding_dim: 8', '"cat_1" num_buckets: 3 embedding_dim: 4'), "sparse group feature dims must be the same"),
    (TEXT.replace("hidden_units: [16, 8]", "hidden_units: [16, 7]"), "dense mlp last hidden_unit must be the same sparse feature dim"),
    (TEXT.replace("model_config {", SEQ_FEATURE).replace('feature_names: "cat_3"\n        group_type: DEEP', 'feature_names: "cat_3"\n' + SEQ_GROUP),
     "sparse group not have sequence features"),
    (TEXT.replace("model_config {", SEQ_FEATURE).replace('feature_names: "int_1"\n        group_type: DEEP', 'feature_names: "int_1"\n' + SEQ_GROUP),
     "dense group not have sequence features"),
])
def test_the_references_refusals(text, message):
    assert text != TEXT
    with pytest.raises(Exception, match=message):
        build_rank_model(load_pipeline_spec(text), device=torch.device("cpu"))


def test_a_config_without_layers_is_refused():
    import re

    gone = re.sub(r"        wukong_layers \{.*?\n        \}\n", "", TEXT, flags=re.S)
    assert "wukong {" in gone and "wukong_layers" not in gone and "final {" in gone
    with pytest.raises(ValueError, match="wukong_layers"):
        build_rank_model(load_pipeline_spec(gone), device=torch.device("cpu"))


@pytest.mark.parametrize("text,field", [
    (TEXT.replace("final {", "finall {"), "finall"),  # (missing, and unknown: named either way)
    (TEXT.replace("lcb_feature_num: 3", ""), "lcb_feature_num"),
    (TEXT.replace("fmb_feature_num: 4", ""), "fmb_feature_num"),
    (TEXT.replace("lcb_feature_num: 3", "lcb_feature_num: 3 dropout: 0.1"), "dropout"),
    (TEXT.replace("fmb_feature_num: 4", "fmb_feature_num: 4 use_residual: true"), "use_residual"),
    (TEXT.replace("feature_num_mlp {\n                hidden_units: [12]\n            }", "", 1), "feature_num_mlp"),
    (TEXT.replace("dense_mlp {", "dense_mlpp {"), "dense_mlpp"),
])
def test_config_errors_name_the_field(text, field):
    assert text != TEXT
    with pytest.raises(ValueError, match=field):
        build_rank_model(load_pipeline_spec(text), device=torch.device("cpu"))
