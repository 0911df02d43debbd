"""`sequence_groups` / `sequence_encoders` of a DEEP feature group (tzrec/modules/embedding.py:196-383, 529-536): the loader
keeps and validates the two blocks, EmbeddingGroup builds the nested sequence group's tables and the encoder modules, and the
group's tensor is cat(own features, encoder 0, encoder 1, ...).  tests/golden/mmoe_seq_mini.config: the reference's
mmoe_has_sequence at test size, with all three encoder kinds this project builds on the one sequence group."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from torcheasyrec_amd.config import SeqEncoderSpec, SeqGroupSpec, load_pipeline_spec, parse_text_proto  # noqa: E402
from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch  # noqa: E402
from torcheasyrec_amd.rank_model import build_rank_model  # noqa: E402
from torcheasyrec_amd.sequence import DINEncoder, PoolingEncoder, SimpleAttention  # noqa: E402
from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MINI = os.path.join(HERE, "golden", "mmoe_seq_mini.config")
SEQ_LENS = [0, 8, 3, 1, 8, 5, 11, 2]  # no history, the full sequence_length, one longer than it (truncated to 8)


def mini_text():
    return open(MINI).read()


def mini_batch(spec, lens=SEQ_LENS, seed=0):
    """hand-built: one id per plain feature, the click history of SEQ_LENS for both sub-features of click_seq"""
    rng = np.random.default_rng(seed)
    B = len(lens)
    sparse = [f for f in spec.features if f.is_sparse]
    dense = [f for f in spec.features if not f.is_sparse]
    ln = [np.asarray(lens, np.int32) if f.is_sequence else np.ones(B, np.int32) for f in sparse]
    ids = [rng.integers(0, f.num_embeddings, size=int(l.sum())).astype(np.int64) for f, l in zip(sparse, ln)]
    kjt = KeyedJaggedTensor([f.name for f in sparse], torch.from_numpy(np.concatenate(ids)), torch.from_numpy(np.concatenate(ln)))
    kt = KeyedTensor([f.name for f in dense], [f.value_dim for f in dense], torch.from_numpy(rng.random((B, len(dense)), dtype=np.float32)))
    labels = {n: torch.from_numpy((rng.random(B) < 0.4).astype(np.int64)) for n in spec.label_fields}
    return Batch({BASE_DATA_GROUP: kt}, {BASE_DATA_GROUP: kjt}, labels), dict(zip([f.name for f in sparse], ids))


def test_loader_keeps_sequence_groups_and_encoders():
    spec = load_pipeline_spec(mini_text())
    (g,) = spec.feature_groups
    assert g.group_name == "all" and g.group_type == "DEEP" and g.feature_names == ["user_id", "adgroup_id", "cate_id", "price"]
    assert g.sequence_groups == [SeqGroupSpec("click_seq", ["adgroup_id", "cate_id", "click_seq__adgroup_id", "click_seq__cate_id"], None)]
    assert g.sequence_encoders == [
        SeqEncoderSpec("din_encoder", "click_seq", 0, {"hidden_units": [8, 4]}, "mean"),  # (an encoder without `input`: the only group)
        SeqEncoderSpec("simple_attention", "click_seq", 0, None, "mean"),
        SeqEncoderSpec("pooling_encoder", "click_seq", 0, None, "mean")]
    # a single unnamed sequence group takes the parent's name; the parent's embedding_name_suffix is inherited; fields are read
    text = mini_text().replace('            group_name: "click_seq"\n', "").replace("group_type: DEEP", 'group_type: DEEP embedding_name_suffix: "v2"') \
        .replace("simple_attention { }", "simple_attention { max_seq_length: 5 }").replace('pooling_type: "mean"', 'pooling_type: "sum" max_seq_length: 6')
    g = load_pipeline_spec(text).feature_groups[0]
    assert g.sequence_groups[0].group_name == "all" and g.sequence_groups[0].embedding_name_suffix == "v2"
    assert [e.input for e in g.sequence_encoders] == ["all"] * 3
    assert g.sequence_encoders[1].max_seq_length == 5 and (g.sequence_encoders[2].pooling_type, g.sequence_encoders[2].max_seq_length) == ("sum", 6)


def _with(text, old, new):
    assert old in text
    return text.replace(old, new)


def test_loader_refuses_what_it_cannot_build():
    text = mini_text()
    for kind in ("self_attention_encoder { multihead_attn_dim: 32 num_heads: 2 }", "multi_window_din_encoder { attn_mlp { hidden_units: [8] } windows_len: [2, 4] }",
                 "made_up_encoder { }"):
        with pytest.raises(NotImplementedError, match=kind.split(" ")[0]):  # (never dropped silently: the kind is named)
            load_pipeline_spec(_with(text, "simple_attention { }", kind))
    no_encoders = text
    for e in ("        sequence_encoders { din_encoder { attn_mlp { hidden_units: [8, 4] } } }\n", "        sequence_encoders { simple_attention { } }\n",
              '        sequence_encoders { pooling_encoder { pooling_type: "mean" } }\n'):
        no_encoders = _with(no_encoders, e, "")
    with pytest.raises(ValueError, match="no sequence_encoders"):
        load_pipeline_spec(no_encoders)
    with pytest.raises(ValueError, match="DEEP"):  # the two blocks in a WIDE group
        load_pipeline_spec(_with(text, "group_type: DEEP", "group_type: WIDE"))
    second = '        sequence_groups { group_name: "other" feature_names: "adgroup_id" feature_names: "click_seq__cate_id" }\n'
    with pytest.raises(ValueError, match="needs an `input`"):  # several groups: encoders must say which one they read
        load_pipeline_spec(_with(text, "        sequence_encoders { din_encoder", second + "        sequence_encoders { din_encoder"))
    named = _with(text, "din_encoder { attn_mlp", 'din_encoder { input: "click_seq" attn_mlp')
    named = _with(_with(named, "simple_attention { }", 'simple_attention { input: "click_seq" }'), 'pooling_encoder { pooling_type', 'pooling_encoder { input: "click_seq" pooling_type')
    with pytest.raises(ValueError, match="other has no sequence encoder"):  # every group needs an encoder
        load_pipeline_spec(_with(named, "        sequence_encoders { din_encoder", second + "        sequence_encoders { din_encoder"))
    with pytest.raises(ValueError, match="none of its sequence_groups"):
        load_pipeline_spec(_with(named, 'simple_attention { input: "click_seq" }', 'simple_attention { input: "nowhere" }'))
    unnamed = _with(text, '            group_name: "click_seq"\n', "")
    with pytest.raises(ValueError, match="needs a group_name"):  # several groups need names
        load_pipeline_spec(_with(unnamed, "        sequence_encoders { din_encoder", second + "        sequence_encoders { din_encoder"))


def test_existing_configs_parse_as_before():
    """no config without the two blocks parses differently: the four fields a feature group had come straight from the text,
    the two new ones are empty"""
    paths = [p for p in glob.glob(os.path.join(HERE, "golden", "**", "*.config"), recursive=True) if os.path.basename(p) != "mmoe_seq_mini.config"]
    assert len(paths) >= 7
    for path in paths:
        text = open(path).read()
        spec = load_pipeline_spec(text)
        raw = parse_text_proto(text).one("model_config").many("feature_groups")
        assert len(raw) == len(spec.feature_groups) > 0, path
        for g, m in zip(spec.feature_groups, raw):
            assert (g.group_name, g.feature_names, g.group_type, g.embedding_name_suffix) == (
                m.one("group_name"), list(m.many("feature_names")), str(m.one("group_type", "DEEP")), m.one("embedding_name_suffix")), path
            assert g.sequence_groups == [] and g.sequence_encoders == [], path


def _expected_group(model, batch, ids):
    """cat(pooled group, the three encoders' PADDED forms) from the tables' own rows, indexed by hand"""
    eg = model.embedding_group
    pooled, seq = eg.ebc.table_weights(), eg.ecs["16"].table_weights()
    price = batch.dense_features[BASE_DATA_GROUP].values()
    own = torch.cat([pooled[f"{n}_emb"].detach()[torch.from_numpy(ids[n])] for n in ("user_id", "adgroup_id", "cate_id")] + [price], dim=1)
    B, L = len(SEQ_LENS), 8
    query = torch.cat([seq[f"{n}_emb"].detach()[torch.from_numpy(ids[n])] for n in ("adgroup_id", "cate_id")], dim=1)
    padded = torch.zeros(B, L, 32, device=own.device)
    start = 0
    for b, n in enumerate(SEQ_LENS):
        k = min(n, L)
        for j, name in enumerate(("click_seq__adgroup_id", "click_seq__cate_id")):
            padded[b, :k, 16 * j:16 * (j + 1)] = seq[f"{name}_emb"].detach()[torch.from_numpy(ids[name][start:start + k])]
        start += n
    d = {"click_seq.query": query, "click_seq.sequence": padded,
         "click_seq.sequence_length": torch.tensor(SEQ_LENS, dtype=torch.int64, device=own.device)}
    encs = eg._group_name_to_seq_encoders["all"]
    with torch.no_grad():
        return torch.cat([own] + [enc(d) for enc in encs], dim=1), query


def test_group_tensor_and_training_step(dev):
    spec = load_pipeline_spec(mini_text())
    torch.manual_seed(2)
    model = build_rank_model(spec, device=dev)
    eg = model.embedding_group
    # tables: the nested group's features are looked up unpooled through tables of their own (as a SEQUENCE group's)
    assert sorted(eg.ecs["16"].table_weights()) == ["adgroup_id_emb", "cate_id_emb", "click_seq__adgroup_id_emb", "click_seq__cate_id_emb"]
    encs = eg._group_name_to_seq_encoders["all"]
    assert [type(e) for e in encs] == [DINEncoder, SimpleAttention, PoolingEncoder] and all(e.input() == "click_seq" for e in encs)
    assert any(k.startswith("embedding_group._group_name_to_seq_encoders.all.0.mlp.") for k in model.state_dict())  # the reference's keys
    own = 16 + 16 + 16 + 1
    assert eg.group_total_dim("all") == own + 3 * 32
    assert eg.group_dims("all") == [16, 16, 16, 1, 32, 32, 32]
    assert list(eg.group_feature_dims("all")) == ["user_id", "adgroup_id", "cate_id", "price", "all_seq_encoder_0", "all_seq_encoder_1", "all_seq_encoder_2"]
    assert eg.group_total_dim("click_seq.sequence") == 32 and eg.group_total_dim("click_seq.query") == 32
    # the nested group configures sequence_length and all three encoders evaluate rows: the jagged form is chosen
    assert eg.jagged_sequence_groups == {"click_seq"} and eg.nested_sequence_groups() == ["click_seq"]
    batch, ids = mini_batch(spec)
    batch = batch.to(dev)
    want, query = _expected_group(model, batch, ids)
    model.eval()
    with torch.no_grad():
        out = eg(batch)
        assert "click_seq.sequence_jagged" in out and "click_seq.sequence" not in out
        torch.testing.assert_close(out["all"], want, rtol=1e-5, atol=1e-5)
        assert torch.equal(out["click_seq.query"], query)  # the nested group's .query stays in the dict
        eg.jagged_sequence_groups.clear()  # the padded form of the same group
        out_p = eg(batch)
        assert tuple(out_p["click_seq.sequence"].shape) == (len(SEQ_LENS), 8, 32)
        torch.testing.assert_close(out_p["all"], want, rtol=1e-5, atol=1e-5)
        eg.jagged_sequence_groups.add("click_seq")
    # one training step: the sequence tables' touched rows move (the fused sparse update runs through the nested group) and
    # the DIN tower inside the group has gradients
    model.train()
    seq_tables = {n: w.detach().clone() for n, w in eg.ecs["16"].table_weights().items()}
    dense = list(model.dense_parameters())
    assert any(p_ is encs[0].linear.weight for p_ in dense)  # the encoders' parameters are dense parameters of the model
    sum(model.loss(model(batch), batch).values()).backward()
    for n, before in seq_tables.items():
        after = eg.ecs["16"].table_weights()[n].detach()
        key = n[:-len("_emb")]
        # (a query row only receives a gradient through a softmax over >= 2 positions: with none or one the weights are constant)
        k = torch.from_numpy(ids[key][np.asarray(SEQ_LENS) >= 2]) if not key.startswith("click_seq__") else None
        if key.startswith("click_seq__"):  # positions behind sequence_length (sample 6: 11 ids, 8 kept) receive a zero gradient
            off = np.concatenate([[0], np.cumsum(SEQ_LENS)])
            k = torch.from_numpy(np.concatenate([ids[key][off[b]:off[b] + min(n_, 8)] for b, n_ in enumerate(SEQ_LENS)]))
        touched = torch.zeros(before.shape[0], dtype=torch.bool)
        touched[k] = True
        moved = (after != before).any(dim=1).cpu()
        assert bool(moved[touched].all()), n
        assert not bool(moved[~touched].any()), n
    for p_ in encs[0].parameters():
        assert p_.grad is not None and float(p_.grad.abs().sum()) > 0


def test_encoder_outside_the_kernels_limits_keeps_the_padded_form(dev):
    """a DIN attention MLP whose last width is no multiple of 4 cannot run on rows (DINEncoder.jagged_limit): the nested group
    stays padded, for all of its encoders"""
    text = _with(mini_text(), "hidden_units: [8, 4] } } }", "hidden_units: [8, 6] } } }")
    model = build_rank_model(load_pipeline_spec(text), device=dev)
    assert model.embedding_group.jagged_sequence_groups == set()
    spec = load_pipeline_spec(text)
    batch, _ = mini_batch(spec)
    out = model.embedding_group(batch.to(dev))
    assert "click_seq.sequence" in out and out["all"].shape[1] == 49 + 96


def test_nested_group_name_may_not_be_another_groups_name():
    text = _with(mini_text(), "    mmoe {", '    feature_groups { group_name: "click_seq" feature_names: "user_id" group_type: DEEP }\n    mmoe {')
    with pytest.raises(ValueError, match="another group"):
        build_rank_model(load_pipeline_spec(text), device=torch.device("cpu"))
