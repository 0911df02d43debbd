"""`mask_net {...}` from its config (tests/golden/masknet_mini.config): the model the reference builds from the same file
(tzrec/models/masknet.py:25-65), its LayerNorms, masks and concat on csrc/ln_mask.hip."""
import itertools
import os

import pytest
import torch

import masknet_ref as ref
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import _lib
from torcheasyrec_amd import masknet
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.dense_optim import build_dense_optimizer, named_dense_parameters
from torcheasyrec_amd.embedding_group import TrainPipeline
from torcheasyrec_amd.masknet import MaskNetModule
from torcheasyrec_amd.optimizer import build_train_optimizer
from torcheasyrec_amd.rank_model import ConfigMaskNet, build_rank_model

TEXT = open(os.path.join(os.path.dirname(__file__), "golden", "masknet_mini.config")).read()
BLOCK = "reduction_ratio: 1.5\n                hidden_dim: 24"
TOP = "top_mlp {\n                hidden_units: [16, 8]\n            }"


def _perturb_layer_norms(model, dev):
    with torch.no_grad():  # (the reference's weight 1 and bias 0 would hide gamma and beta)
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_((1.0 + 0.3 * torch.randn(m.weight.shape)).to(dev))
                m.bias.copy_((0.3 * torch.randn(m.bias.shape)).to(dev))


def _model(dev, seed=0, text=TEXT):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    model = build_rank_model(spec, device=dev)
    _perturb_layer_norms(model, dev)
    return spec, model


def test_config_builds_the_references_model(dev):
    assert BLOCK in TEXT and TOP in TEXT
    spec, model = _model(dev)
    assert spec.model_name == "mask_net" and type(model) is ConfigMaskNet
    assert model.embedding_group.group_total_dim("all") == 69  # four 16-wide id features + raw features of width 5: odd
    mn = model.mask_net_layer
    assert isinstance(mn, MaskNetModule) and mn.use_parallel and len(mn.mask_blocks) == 3 and mn.output_dim() == 8
    assert [b.aggregation_dim for b in mn.mask_blocks] == [103] * 3  # int(69 * 1.5)
    keys = set(model.state_dict())
    dense = {k for k in keys if not k.startswith("embedding_group.")}
    block = ["mask_generator.0.weight", "mask_generator.0.bias", "mask_generator.2.weight", "mask_generator.2.bias",
             "ffn.0.weight", "ffn.0.bias", "ffn.1.weight", "ffn.1.bias"]
    assert dense == {"mask_net_layer.ln_emb.weight", "mask_net_layer.ln_emb.bias", "output_linear.weight"} \
        | {f"mask_net_layer.mask_blocks.{i}.{k}" for i in range(3) for k in block} \
        | {f"mask_net_layer.top_mlp.mlp.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")}
    assert "output_linear.bias" not in keys and model.output_linear.weight.shape == (1, 8)
    assert mn.top_mlp.mlp[0].in_features == 3 * 24
    # the parameter count: ln_emb, per block the mask generator (69 -> 103 -> 69), the hidden layer (69 -> 24) and its LayerNorm,
    # the top MLP (72 -> 16 -> 8), the logits layer without bias
    per_block = (69 * 103 + 103) + (103 * 69 + 69) + (69 * 24 + 24) + 2 * 24
    want = 2 * 69 + 3 * per_block + (72 * 16 + 16) + (16 * 8 + 8) + 8
    assert sum(p.numel() for p in model.dense_parameters()) == want and len(list(model.dense_parameters())) == len(dense) == 31
    # serial blocks, the configured aggregation_dim with reduction_ratio 0, the defaults
    ser = _model(dev, text=TEXT.replace("use_parallel: true", "use_parallel: false"))[1].mask_net_layer
    assert not ser.use_parallel and [b.aggregation_dim for b in ser.mask_blocks] == [103, 36, 36] and ser.top_mlp.mlp[0].in_features == 24
    agg = _model(dev, text=TEXT.replace("reduction_ratio: 1.5", "reduction_ratio: 0 aggregation_dim: 7"))[1].mask_net_layer
    assert [b.aggregation_dim for b in agg.mask_blocks] == [7] * 3
    both = _model(dev, text=TEXT.replace("reduction_ratio: 1.5", "reduction_ratio: 1.5 aggregation_dim: 7"))[1].mask_net_layer
    assert [b.aggregation_dim for b in both.mask_blocks] == [103] * 3
    dflt = _model(dev, text=TEXT.replace("reduction_ratio: 1.5", "").replace("use_parallel: true", ""))[1].mask_net_layer
    assert dflt.use_parallel and [b.aggregation_dim for b in dflt.mask_blocks] == [69] * 3


@pytest.mark.parametrize("text,field", [
    (TEXT.replace("mask_net_module {", "mask_net_modul {"), "mask_net_modul"),  # (missing, and unknown: named either way)
    (TEXT.replace("n_mask_blocks: 3", ""), "n_mask_blocks"),
    (TEXT.replace("mask_block {", "mask_blocc {"), "mask_blocc"),
    (TEXT.replace(BLOCK, "reduction_ratio: 1.5"), "hidden_dim"),
    (TEXT.replace(TOP, ""), "top_mlp"),
    (TEXT.replace(TOP, "top_mlp {\n            }"), "top_mlp"),
    (TEXT.replace("use_parallel: true", "use_parallel: true use_serial: true"), "use_serial"),
    (TEXT.replace("hidden_dim: 24", "hidden_dim: 24 dropout: 0.1"), "dropout"),
    (TEXT.replace("reduction_ratio: 1.5", "reduction_ratio: 0"), "aggregation_dim or reduction_ratio"),
])
def test_config_errors_name_the_field(text, field):
    with pytest.raises(ValueError, match=field):
        build_rank_model(load_pipeline_spec(text), device=torch.device("cpu"))


def test_missing_blocks_are_named():
    import re

    gone = re.sub(r"mask_net_module \{.*?use_parallel: true\n        \}\n", "", TEXT, flags=re.S)
    assert "mask_net {" in gone and "mask_net_module" not in gone
    with pytest.raises(ValueError, match="mask_net_module"):
        build_rank_model(load_pipeline_spec(gone), device=torch.device("cpu"))
    gone = re.sub(r"mask_block \{.*?hidden_dim: 24\n            \}\n", "", TEXT, flags=re.S)
    assert "mask_block {" not in gone
    with pytest.raises(ValueError, match="mask_block"):
        build_rank_model(load_pipeline_spec(gone), device=torch.device("cpu"))


def _recompose(features, model, dtype):
    """logits from the group's features and the model's parameters in plain torch on the CPU: the literal module
    (tests/masknet_ref.py), the top MLP (Linear + ReLU), the logits layer without bias"""
    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items() if not k.startswith("embedding_group.")}
    mn = {k[len("mask_net_layer."):]: v for k, v in sd.items() if k.startswith("mask_net_layer.") and ".top_mlp." not in k}
    x = features.detach().cpu().to(dtype)
    h = ref.masknet_literal(x, mn, 3, True, torch.zeros(x.shape[0], 72), dtype)["y"][0]
    for i in (0, 2):
        h = torch.relu(torch.nn.functional.linear(h, sd[f"mask_net_layer.top_mlp.mlp.{i}.weight"], sd[f"mask_net_layer.top_mlp.mlp.{i}.bias"]))
    return torch.nn.functional.linear(h, sd["output_linear.weight"]).squeeze(1)


def test_forward_is_the_recomposition_with_the_literal_module(dev):
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


def _train(dev, steps):
    """the loop of examples/train_from_config.py over one batch seen `steps` times"""
    spec, model = _model(dev, seed=3)
    opt = build_dense_optimizer(named_dense_parameters(model), spec.dense_optimizer)
    pipe = TrainPipeline(model, build_train_optimizer(opt, spec.grad_clipping, spec.gradient_accumulation_steps), dev, model.loss)
    batch = next(synthetic_batches(spec, 128, 128, seed=4))
    it, losses = itertools.repeat(batch, steps), []
    for _ in range(steps):
        l, _, _ = pipe.progress(it)
        assert list(l) == ["binary_cross_entropy"]  # keyed by the config's own loss name
        losses.append(float(l["binary_cross_entropy"].detach()))
    return losses, model


def test_a_few_steps_bring_the_loss_down(dev, monkeypatch):
    """five steps over one batch: finite losses, none above the one before, under the config's loss name; the row kernels ran
    twice per step each way; the literal twin's losses agree to rtol = atol = 1e-5 (what tests/test_dcn_config.py holds a step to)"""
    lib, calls = _lib.lib(), [0, 0]
    fwd, bwd = lib.tzr_ln_mask_fwd, lib.tzr_ln_mask_bwd

    def cf(*a):
        calls[0] += 1
        return fwd(*a)

    def cb(*a):
        calls[1] += 1
        return bwd(*a)

    lib.tzr_ln_mask_fwd, lib.tzr_ln_mask_bwd = cf, cb
    try:
        fused, model = _train(dev, 5)
        assert calls == [10, 10]
        monkeypatch.setattr(masknet, "FUSED_MASKNET", False)
        literal, _ = _train(dev, 5)
        assert calls == [10, 10]
    finally:
        lib.tzr_ln_mask_fwd, lib.tzr_ln_mask_bwd = fwd, bwd
    print(f"losses on {dev.type}: fused {fused} literal {literal}")
    assert all(torch.isfinite(torch.tensor(fused))) and all(b <= a for a, b in zip(fused, fused[1:])), fused
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.mask_net_layer.parameters())
    torch.testing.assert_close(torch.tensor(fused), torch.tensor(literal), rtol=1e-5, atol=1e-5)
