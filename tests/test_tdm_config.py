"""`tdm {...}` from its config (tests/golden/tdm_mini.config) on the lane emulator: the model builds with the reference's parameter
names, its forward is the same modules composed literally (the encoder on the padded tensors), two training steps through the
example's batches give finite losses with the encoder's kernel launched, and everything the model does not build is refused by name."""
import os
import sys

import pytest
import torch

from torcheasyrec_amd import _lib
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.rank_model import ConfigTDM, build_rank_model

TEXT = open(os.path.join(os.path.dirname(__file__), "golden", "tdm_mini.config")).read()
# tzrec/models/tdm.py:63-77 over the mini config, the reference's `mlp.<i>.perceptron.0` / `.1` being this package's `mlp.<2i>` / `<2i + 1>`
REFERENCE_KEYS = sorted(
    ["multiwindow_din.windows_len", "multiwindow_din.cumsum_windows_len", "multiwindow_din.linear.weight", "multiwindow_din.linear.bias",
     "multiwindow_din.active.weight", "output_mlp.weight", "output_mlp.bias"]
    + [f"multiwindow_din.mlp.mlp.{i}.{p}" for i, ps in enumerate((("weight", "bias"), ("weight",)) * 2) for p in ps]
    + [f"deep_mlp.mlp.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")]
    + ["embedding_group.ebc.embedding_bags.user_id_emb.weight"]
    + [f"embedding_group.ecs.4._store.embedding_bags.{t}_emb.weight" for t in ("adgroup_id", "cate_id", "click_seq__adgroup_id", "click_seq__cate_id")])


@pytest.fixture
def emu(emu_path):
    _lib.use_library(emu_path)
    return torch.device("cpu")


def build(text):
    spec = load_pipeline_spec(text)
    torch.manual_seed(0)
    return spec, build_rank_model(spec, device=torch.device("cpu"))


def batches(spec, n):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "examples"))
    from train_from_config import synthetic_batches

    return list(synthetic_batches(spec, 33 * n, 33, seed=1))[:n]


def test_builds_with_the_references_names_and_equals_its_modules_composed_literally(emu):
    from torcheasyrec_amd.sequence import _MwdinFn, jagged_to_padded_dense, mwdin_literal

    spec, model = build(TEXT)
    assert type(model) is ConfigTDM and sorted(model.state_dict()) == REFERENCE_KEYS
    assert model.embedding_group.jagged_sequence_groups == {"seq"} and model.multiwindow_din.output_dim() == 6 * 8
    b, before = batches(spec, 1)[0], _MwdinFn.calls
    got = model(b)
    assert _MwdinFn.calls == before + 1 and got["logits"].shape == (33, 2)
    g = model.build_input(b)
    seq = jagged_to_padded_dense(g["seq.sequence_jagged"], g["seq.sequence_offsets"], 20)
    enc = mwdin_literal(g["seq.query"], seq, g["seq.sequence_length"], model.multiwindow_din)
    want = model.output_mlp(model.deep_mlp(torch.cat([enc, g["deep"]], dim=1)))
    assert torch.allclose(got["logits"], want, rtol=1e-5, atol=1e-6)


def test_two_training_steps_give_finite_losses(emu):
    from torcheasyrec_amd.embedding_group import TrainPipeline

    spec, model = build(TEXT)
    pipe = TrainPipeline(model, torch.optim.Adam(list(model.dense_parameters()), lr=1e-2), torch.device("cpu"), model.loss)
    before = model.multiwindow_din.linear.bias.detach().clone()
    it = iter(batches(spec, 2))
    for _ in range(2):
        losses = pipe.progress(it)[0]
        assert list(losses) == ["softmax_cross_entropy"] and bool(torch.isfinite(losses["softmax_cross_entropy"]))
    assert not torch.equal(before, model.multiwindow_din.linear.bias)


REFUSALS = {
    "tdm_sampler": (lambda t: t.replace("num_workers: 1", "num_workers: 1 tdm_sampler { item_input_path: 'x' }"), NotImplementedError, "tree sampler is data-side"),
    "two_sequence_groups": (lambda t: t.replace("    tdm {", "    feature_groups { group_name: 'seq2' feature_names: 'cate_id' feature_names: 'click_seq__cate_id' "
                                                "group_type: SEQUENCE }\n    tdm {"), ValueError, "exactly one SEQUENCE"),
    "unknown_tdm_field": (lambda t: t.replace("final { hidden_units: [16, 8] }", "final { hidden_units: [16, 8] } towers { }"), ValueError, "tdm has no field 'towers'"),
    "unknown_din_field": (lambda t: t.replace("windows_len: [1, 1, 2, 4, 9]", "windows_len: [1] max_seq_length: 3"), ValueError, "multiwindow_din has no field 'max_seq_length'"),
    "empty_windows_len": (lambda t: t.replace("windows_len: [1, 1, 2, 4, 9]", ""), ValueError, "windows_len is empty"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refused_by_name_when_the_model_is_built(emu, name):
    make, exc, words = REFUSALS[name]
    text = make(TEXT)
    assert text != TEXT
    with pytest.raises(exc, match=words):
        build(text)
