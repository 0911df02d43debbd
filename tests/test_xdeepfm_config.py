"""`xdeepfm {...}` from its config (tests/golden/xdeepfm_mini.config): the model the reference builds from the same file
(tzrec/models/xdeepfm.py:44-86), its compressed interaction network on csrc/cin.hip."""
import itertools
import os

import pytest
import torch

import cin_ref as ref
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import interaction
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.dense_optim import build_dense_optimizer, named_dense_parameters
from torcheasyrec_amd.embedding_group import TrainPipeline
from torcheasyrec_amd.interaction import CIN
from torcheasyrec_amd.optimizer import build_train_optimizer
from torcheasyrec_amd.rank_model import ConfigXDeepFM, build_rank_model

HERE = os.path.dirname(__file__)
TEXT = open(os.path.join(HERE, "golden", "xdeepfm_mini.config")).read()


def _model(dev, seed=0, text=TEXT):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=dev)


def test_config_builds_the_references_model(dev):
    spec, model = _model(dev)
    assert spec.model_name == "xdeepfm" and type(model) is ConfigXDeepFM
    eg = model.embedding_group
    assert spec.wide_embedding_dim == 16 and eg.group_dims("wide") == [16] * 4  # the message's default, not DeepFM's 4
    assert eg.group_total_dim("deep") == 4 + 4 * 8
    assert isinstance(model.cin, CIN) and model.cin.feature_num == 4 and model.cin.cin_layer_size == [8, 4] and model.cin.output_dim() == 12
    keys = set(model.state_dict())
    dense = {k for k in keys if not k.startswith("embedding_group.")}
    assert dense == {"cin.cin_layers.0.weight", "cin.cin_layers.0.bias", "cin.cin_layers.1.weight", "cin.cin_layers.1.bias",
                     "deep.mlp.0.weight", "deep.mlp.0.bias", "deep.mlp.2.weight", "deep.mlp.2.bias",
                     "final.mlp.0.weight", "final.mlp.0.bias", "output_mlp.weight", "output_mlp.bias"}
    assert model.cin.cin_layers[0].weight.shape == (8, 16, 1) and model.cin.cin_layers[1].weight.shape == (4, 32, 1)
    assert model.final.mlp[0].in_features == 12 + 16 and model.output_mlp.weight.shape == (1, 8)
    assert len(list(model.dense_parameters())) == len(dense)
    # an explicit wide_embedding_dim is taken; DeepFM's default stays 4
    assert _model(dev, text=TEXT.replace("xdeepfm {", "xdeepfm {\n wide_embedding_dim: 4"))[1].embedding_group.group_dims("wide") == [4] * 4
    deepfm = load_pipeline_spec(open(os.path.join(HERE, "golden", "deepfm_mini.config")).read())
    assert deepfm.wide_embedding_dim == 0  # (the embedding group's fallback of 4)
    # cin is required; an unknown field of the block raises by name
    with pytest.raises(ValueError, match="cin"):
        _model(dev, text=TEXT.replace("cin_layer_size: [8, 4]", "").replace("cin {", "cin_gone {").replace("cin_gone {\n            \n        }", ""))
    with pytest.raises(ValueError, match="split_half"):
        _model(dev, text=TEXT.replace("cin_layer_size: [8, 4]", "cin_layer_size: [8, 4] split_half: true"))


def _recompose(wide, deep_in, model, dtype):
    """logits from the groups' features and the model's parameters in plain torch on the CPU: the literal CIN, the two MLPs
    (Linear + ReLU) over [cin | deep] in that order, the logits layer with bias"""
    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items() if not k.startswith("embedding_group.")}
    x = wide.detach().cpu().to(dtype).reshape(-1, 4, 16)
    cin = ref.literal_forward(x, [sd[f"cin.cin_layers.{i}.weight"] for i in range(2)], [sd[f"cin.cin_layers.{i}.bias"] for i in range(2)])
    deep = deep_in.detach().cpu().to(dtype)
    for i in (0, 2):
        deep = torch.relu(torch.nn.functional.linear(deep, sd[f"deep.mlp.{i}.weight"], sd[f"deep.mlp.{i}.bias"]))
    h = torch.relu(torch.nn.functional.linear(torch.cat([cin, deep], dim=1), sd["final.mlp.0.weight"], sd["final.mlp.0.bias"]))
    return torch.nn.functional.linear(h, sd["output_mlp.weight"], sd["output_mlp.bias"]).squeeze(1)


def test_forward_is_the_recomposition_in_the_order_cin_then_deep(dev):
    spec, model = _model(dev, seed=1)
    batch = next(synthetic_batches(spec, 100, 100, seed=2)).to(dev)
    with torch.no_grad():
        g = model.build_input(batch)
        logits = model(batch)["logits"]
    want = _recompose(g["wide"], g["deep"], model, torch.float64)
    gap = ref.rel_err([_recompose(g["wide"], g["deep"], model, torch.float32)], [want])
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
        assert list(l) == ["binary_cross_entropy"]
        losses.append(float(l["binary_cross_entropy"].detach()))
    return losses, model


def test_training_brings_the_loss_down_and_agrees_with_the_literal_form(dev, monkeypatch):
    """six steps, fused and with FUSED_CIN off: |fused - literal| / max(1, |literal|) <= max(4 x gap, 2^-20) per step, gap = the
    largest distance over the steps between the same run on torch's literal and on torch's factored fp32 form (a third twin
    whose CIN.forward is tests/cin_ref.py's) -- two associations of the same math, neither computed by the kernels"""
    from torcheasyrec_amd import _lib

    steps, lib, calls = 6, _lib.lib(), [0]
    fwd = lib.tzr_cin_fwd

    def counted(*a):
        calls[0] += 1
        return fwd(*a)

    lib.tzr_cin_fwd = counted
    try:
        fused, model = _train(dev, steps)
        assert calls[0] == steps
        assert fused[-1] < fused[0], fused
        assert all(float(p.grad.abs().max()) > 0 for p in model.cin.parameters())
        monkeypatch.setattr(interaction, "FUSED_CIN", False)
        literal, _ = _train(dev, steps)
        assert calls[0] == steps
    finally:
        lib.tzr_cin_fwd = fwd
    monkeypatch.setattr(CIN, "forward", lambda self, x: ref.factored_forward(x, [l.weight for l in self.cin_layers], [l.bias for l in self.cin_layers]))
    factored, _ = _train(dev, steps)
    gap = max(abs(a - b) / max(1.0, abs(a)) for a, b in zip(literal, factored))
    bound = max(4.0 * gap, ref.FLOOR)
    errs = [abs(a - b) / max(1.0, abs(b)) for a, b in zip(fused, literal)]
    print(f"losses on {dev.type}: fused {fused} literal {literal} factored {factored} errs {errs} gap {gap:.3e} bound {bound:.3e}")
    assert all(e <= bound for e in errs)
