"""Read tzrec pipeline configs (protobuf text format) without protoc / generated *_pb2 modules.

The reference loads ``examples/*.config`` with ``text_format.Merge`` into ``EasyRecConfig``
(/root/reference/tzrec/utils/config_util.py:25-48); the generated ``tzrec/protos/*_pb2.py`` cannot
be produced here (no protoc).  The hot path only needs the few fields listed
in SURVEY.md section 8 (feature_configs, model_config.feature_groups, the dlrm/deepfm blocks,
train_config.sparse_optimizer, data_config.batch_size), so this module parses the text format
generically and extracts those.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Any, List, Optional

from .dense_opt_kinds import DENSE_KINDS, group_options
from .embedding import SparseOptimizerConfig

_TOKEN = re.compile(r'\s*(?:(#[^\n]*)|("(?:\\.|[^"\\])*")|([{}\[\]:,;<>])|([^\s{}\[\]:,;<>"]+))')


class Msg(dict):
    """A parsed message: field name -> list of values (scalars or Msg), in file order."""

    def one(self, key: str, default: Any = None) -> Any:
        v = self.get(key)
        return v[-1] if v else default

    def many(self, key: str) -> List[Any]:
        return self.get(key, [])

    def has(self, key: str) -> bool:
        return key in self


def _scalar(tok: str) -> Any:
    if tok.startswith('"') or tok.startswith("'"):  # text format allows either quote
        return bytes(tok[1:-1], "utf-8").decode("unicode_escape")
    if tok in ("true", "True"):
        return True
    if tok in ("false", "False"):
        return False
    try:
        return int(tok)
    except ValueError:
        pass
    try:
        return float(tok)
    except ValueError:
        return tok  # enum identifier


def parse_text_proto(text: str) -> Msg:
    toks: List[str] = []
    pos = 0
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            if text[pos:].strip() == "":
                break
            raise ValueError(f"cannot tokenize config at offset {pos}: {text[pos:pos + 30]!r}")
        pos = m.end()
        if m.group(1):
            continue
        toks.append(m.group(2) or m.group(3) or m.group(4))
    i = 0

    def parse_msg(end: Optional[str]) -> Msg:
        nonlocal i
        out = Msg()
        while i < len(toks):
            t = toks[i]
            if t == end:
                i += 1
                return out
            if t in (",", ";"):
                i += 1
                continue
            name = t
            i += 1
            if i < len(toks) and toks[i] == ":":
                i += 1
            t = toks[i]
            if t in ("{", "<"):
                i += 1
                out.setdefault(name, []).append(parse_msg("}" if t == "{" else ">"))
            elif t == "[":
                i += 1
                while toks[i] != "]":
                    if toks[i] == ",":
                        i += 1
                        continue
                    if toks[i] == "{":
                        i += 1
                        out.setdefault(name, []).append(parse_msg("}"))
                    else:
                        out.setdefault(name, []).append(_scalar(toks[i]))
                        i += 1
                i += 1
            else:
                out.setdefault(name, []).append(_scalar(t))
                i += 1
        if end is not None:
            raise ValueError("unbalanced braces in config")
        return out

    return parse_msg(None)


@dataclass
class FeatureSpec:
    """What the hot path needs from a tzrec feature (tzrec/features/feature.py:586-662,
    id_feature.py:52-87, raw_feature.py:35-48)."""

    name: str
    kind: str  # "id_feature" | "raw_feature" | ...
    is_sparse: bool
    embedding_dim: int = 0
    num_embeddings: int = 0
    embedding_name: Optional[str] = None
    pooling: str = "sum"
    value_dim: int = 1
    trainable: bool = True
    is_sequence: bool = False  # sub-feature of a `sequence_feature` block, named <sequence_name>__<feature_name>
    sequence_length: int = 0
    data_type: str = "FP32"  # feature config `data_type` (FP32 | FP16)
    zch: Optional[Msg] = None  # the raw `zch {...}` block (see zch.zch_config_from_msg)
    # `embedding_constraints { sharding_types: ... }` (feature.proto:6-13, features/feature.py:832-845)
    sharding_types: List[str] = field(default_factory=list)


@dataclass
class SeqGroupSpec:
    """One `sequence_groups` entry of a DEEP feature group (protos/model.proto:21-27)"""

    group_name: str
    feature_names: List[str]
    embedding_name_suffix: Optional[str] = None


SEQ_ENCODER_KINDS = ("din_encoder", "simple_attention", "pooling_encoder")  # of protos/seq_encoder.proto:63-71, the ones built


@dataclass
class SeqEncoderSpec:
    """One `sequence_encoders` entry (protos/seq_encoder.proto:6-35)"""

    kind: str  # one of SEQ_ENCODER_KINDS
    input: str  # the sequence group it reads
    max_seq_length: int = 0
    attn_mlp: Optional[dict] = None  # din_encoder: {"hidden_units": [...]}
    pooling_type: str = "mean"  # pooling_encoder: sum | mean


@dataclass
class FeatureGroupSpec:
    group_name: str
    feature_names: List[str]
    group_type: str = "DEEP"  # DEEP | WIDE | SEQUENCE
    embedding_name_suffix: Optional[str] = None
    # a DEEP group's nested sequences: every encoder reduces its group's [B, L, D] to [B, D'], and the group's tensor is
    # cat(own features, encoder 0, encoder 1, ...) (tzrec/modules/embedding.py:196-306, 529-536)
    sequence_groups: List[SeqGroupSpec] = field(default_factory=list)
    sequence_encoders: List[SeqEncoderSpec] = field(default_factory=list)


@dataclass
class DenseOptimizerConfig:
    """`train_config.dense_optimizer`, or one of its `part_optimizers` (protos/optimizer.proto:31-68)"""

    kind: str  # a key of dense_opt_kinds.DENSE_KINDS
    fields: dict = field(default_factory=dict)  # every field of the kind's message, the proto's defaults filled in
    learning_rate: Optional[Msg] = None  # the block itself: its `learning_rate` oneof is lr_scheduler.create_scheduler's to read
    regex_pattern: Optional[str] = None  # a part: the parameter names it takes (re.fullmatch)
    parts: List["DenseOptimizerConfig"] = field(default_factory=list)


# the `metric` oneof of protos/metric.proto:53-66 with each member's defaults (metric.proto:4-51); `grouping_key` is required
METRIC_DEFAULTS = {
    "auc": {"thresholds": 200},
    "multiclass_auc": {"thresholds": 200, "average": "macro"},
    "recall_at_k": {"top_k": 5},
    "mean_absolute_error": {},
    "mean_squared_error": {},
    "accuracy": {"threshold": 0.5, "top_k": 1},
    "grouped_auc": {},
    "xauc": {"sample_ratio": 1e-3, "in_batch": False},
    "grouped_xauc": {"max_pairs_per_group": 100},
    "normalized_entropy": {"eta": 1e-12},
}


@dataclass
class MetricSpec:
    """One `metrics { ... }` entry of the model config or of a task tower (protos/metric.proto:53-66,
    tzrec/models/rank_model.py:264-334, multi_task_rank.py:144-161): the oneof's member and its fields as written, the proto's
    defaults filled in.  Read for every kind; which kinds are BUILT is metrics.Evaluator's to say."""

    kind: str
    fields: dict = field(default_factory=dict)
    tower: Optional[str] = None  # a task tower's metric: its tower_name
    label: Optional[str] = None  # the label it is measured against (the tower's label_name, else the first label field)

    @property
    def suffix(self) -> str:
        return f"_{self.tower}" if self.tower else ""

    @property
    def name(self) -> str:  # the key of the reference's metric dict
        return self.kind + self.suffix


def _metric_specs(blocks, tower: Optional[str], label: Optional[str]) -> List[MetricSpec]:
    out = []
    for m in blocks:
        for kind, body in m.items():
            given = {k: v[-1] for k, v in body[-1].items()} if isinstance(body[-1], Msg) else {}
            if kind == "grouped_auc" and not given.get("grouping_key"):  # (a `required` field of a kind that is built)
                raise ValueError(f"metrics: {kind} needs a grouping_key")
            out.append(MetricSpec(kind=str(kind), fields={**METRIC_DEFAULTS.get(kind, {}), **given}, tower=tower, label=label))
    return out


# the `loss` oneof of protos/loss.proto:4-11 with each member's defaults (loss.proto:44-63); jrc_loss's `session_name` is required
LOSS_DEFAULTS = {
    "binary_cross_entropy": {"label_smoothing": 0.0},
    "softmax_cross_entropy": {"label_smoothing": 0.0},
    "l2_loss": {},
    "jrc_loss": {"alpha": 0.5},
    "binary_focal_loss": {"gamma": 2.0, "alpha": 0.5},
}
SID_LOSS_KINDS = ("recon_loss", "commitment_loss", "contrastive_loss")  # the `sid_loss` oneof (loss.proto:15-19): not built


@dataclass
class LossSpec:
    """One `losses { ... }` entry of the model config or of a task tower (protos/loss.proto:4-11, tzrec/models/rank_model.py:181-262,
    multi_task_rank.py:80-142): the oneof's member and its fields as written, the proto's defaults filled in."""

    kind: str
    fields: dict = field(default_factory=dict)
    tower: Optional[str] = None  # a task tower's loss: its tower_name

    @property
    def suffix(self) -> str:
        return f"_{self.tower}" if self.tower else ""

    @property
    def name(self) -> str:  # the key of the reference's loss dict
        return self.kind + self.suffix


@dataclass
class TowerSpec:
    """What the losses read of a `task_towers` entry (protos/tower.proto:26-57), the proto's defaults filled in."""

    tower_name: str
    label_name: str
    num_class: int = 1
    weight: float = 1.0
    sample_weight_name: Optional[str] = None
    task_space_indicator_label: Optional[str] = None
    in_task_space_weight: float = 1.0
    out_task_space_weight: float = 1.0

    @property
    def has_weight(self) -> bool:  # MultiTaskRank.has_weight (multi_task_rank.py:67-78); a written `weight: 1.0` multiplies by one
        return bool(self.sample_weight_name) or self.weight != 1.0 or bool(self.task_space_indicator_label)


# the model_config oneof's match (retrieval) members (protos/model.proto:71-76): their softmax_cross_entropy runs over the
# similarity scores of one positive and its negatives, not over `num_class` logits (tzrec/models/match_model.py:281-336)
MATCH_MODELS = ("dssm", "dssm_v2", "dat", "hstu_match", "mind")
# data_config's `sampler` oneof (protos/data.proto:160-166)
SAMPLER_KINDS = ("negative_sampler", "negative_sampler_v2", "hard_negative_sampler", "hard_negative_sampler_v2", "tdm_sampler")


def _loss_specs(blocks, tower: Optional[str], num_class: int, sparse_names, match: bool = False) -> List[LossSpec]:
    """The entries of `losses` blocks, refused or validated here, when the spec is built; no block: one plain BCE (what every
    model computed before the block was read).  `match`: the model block is a match model, whose softmax_cross_entropy has
    `num_class: 1`."""
    where = f"task tower {tower}" if tower else "model_config"
    out = []
    for m in blocks:
        for kind, body in m.items():
            if kind not in LOSS_DEFAULTS:
                raise NotImplementedError(f"{where}: loss {kind!r} is not built (built: {', '.join(LOSS_DEFAULTS)})")
            given = {k: v[-1] for k, v in body[-1].items()} if isinstance(body[-1], Msg) else {}
            out.append(LossSpec(kind=str(kind), fields={**LOSS_DEFAULTS[kind], **given}, tower=tower))
    if not out:
        out.append(LossSpec(kind="binary_cross_entropy", fields=dict(LOSS_DEFAULTS["binary_cross_entropy"]), tower=tower))
    for ls in out:
        kind, f = ls.kind, ls.fields
        if kind in ("binary_cross_entropy", "binary_focal_loss") and num_class != 1:
            raise ValueError(f"{where}: num_class must be 1 when loss type is {kind} (got {num_class})")
        if kind == "softmax_cross_entropy" and num_class <= 1 and not match:
            raise ValueError(f"{where}: num_class must be greater than 1 when loss type is {kind} (got {num_class})")
        if kind == "jrc_loss":
            if num_class != 2:
                raise ValueError(f"{where}: num_class must be 2 when loss type is {kind} (got {num_class})")
            if not f.get("session_name"):
                raise ValueError(f"{where}: jrc_loss needs a session_name")
            if str(f["session_name"]) not in sparse_names:
                raise ValueError(f"{where}: jrc_loss session_name {f['session_name']!r} is not a sparse feature of the config")
        if kind == "binary_focal_loss":
            if not float(f["gamma"]) >= 0:
                raise ValueError(f"{where}: binary_focal_loss gamma should be greater than or equal to zero (got {f['gamma']})")
            if not 0 < float(f["alpha"]) < 1:
                raise ValueError(f"{where}: binary_focal_loss alpha should be in (0, 1) (got {f['alpha']})")
    return out


@dataclass
class PipelineSpec:
    features: List[FeatureSpec] = field(default_factory=list)
    feature_groups: List[FeatureGroupSpec] = field(default_factory=list)
    model_name: str = ""
    model: Msg = field(default_factory=Msg)
    wide_embedding_dim: int = 0
    num_class: int = 1
    batch_size: int = 0
    sparse_optimizer: Optional[SparseOptimizerConfig] = None
    dense_lr: float = 1e-3
    dense_optimizer: Optional[DenseOptimizerConfig] = None
    label_fields: List[str] = field(default_factory=list)
    # the raw optimizer blocks (learning-rate schedules: lr_scheduler.create_scheduler)
    sparse_optimizer_block: Optional[Msg] = None
    dense_optimizer_block: Optional[Msg] = None
    # train_config.delta_embedding_dump_config (train.proto:86-111), as parsed (Msg)
    delta_embedding_dump_config: Optional[object] = None
    # train_config.global_embedding_constraints.sharding_types (train.proto:144, plan_util.py:170-179)
    global_sharding_types: List[str] = field(default_factory=list)
    gradient_accumulation_steps: int = 0  # train.proto:151
    grad_clipping: Optional[object] = None  # train.proto:153 -> optimizer.GradClippingConfig
    # model_config.metrics, then every task tower's metrics in tower order (metrics.Evaluator builds them)
    metrics: List[MetricSpec] = field(default_factory=list)
    # model_config.losses (a model without task towers), then every task tower's losses in tower order (losses.build_losses)
    losses: List[LossSpec] = field(default_factory=list)
    task_towers: List[TowerSpec] = field(default_factory=list)
    sample_weight_fields: List[str] = field(default_factory=list)  # data_config.sample_weight_fields
    # data_config.negative_sampler (protos/sampler.proto:5-23) as written, num_sample an int and attr_fields a list; None: none
    negative_sampler: Optional[dict] = None
    sampler_kinds: List[str] = field(default_factory=list)  # the members of data_config's `sampler` oneof that are written
    model_config_keys: List[str] = field(default_factory=list)  # every field written in model_config

    def tower(self, name: Optional[str]) -> Optional[TowerSpec]:
        return next((t for t in self.task_towers if t.tower_name == name), None)


def _num_embeddings(f: Msg, name: str) -> int:
    """IdFeature.num_embeddings precedence (tzrec/features/id_feature.py:64-87)."""
    if f.has("zch"):
        return int(f.one("zch").one("zch_size"))
    if f.has("dynamicemb"):
        return int(f.one("dynamicemb").one("max_capacity"))
    if f.has("hash_bucket_size"):
        return int(f.one("hash_bucket_size"))
    if f.has("num_buckets"):
        return int(f.one("num_buckets"))
    if f.has("vocab_list"):
        return len(f.many("vocab_list"))
    raise ValueError(f"IdFeature[{name}] must set hash_bucket_size or num_buckets or vocab_list or zch.zch_size")


def sparse_optimizer_from_config(opt: Msg) -> SparseOptimizerConfig:
    """create_sparse_optimizer mapping (tzrec/optim/optimizer_builder.py:30-97) for the kinds this
    library fuses (all ten of the oneof); field defaults from protos/optimizer.proto:76-157."""
    table = {"sgd_optimizer": "sgd", "adagrad_optimizer": "adagrad", "rowwise_adagrad_optimizer": "rowwise_adagrad",
             "adam_optimizer": "adam", "partial_rowwise_adam_optimizer": "partial_rowwise_adam",
             "lamb_optimizer": "lamb", "partial_rowwise_lamb_optimizer": "partial_rowwise_lamb",
             "lars_sgd_optimizer": "lars_sgd"}
    # the two kinds with hyper-parameters of their own (protos/optimizer.proto:141-157): eps IS a field of theirs
    if opt.has("adadelta_optimizer") or opt.has("rmsprop_optimizer"):
        kind = "adadelta" if opt.has("adadelta_optimizer") else "rmsprop"
        m = opt.one(f"{kind}_optimizer")
        eps = float(m.one("eps", 1e-6 if kind == "adadelta" else 1e-8))
        if not eps > 0.0:
            raise ValueError(f"{kind}_optimizer: eps must be > 0 (got {eps})")
        return SparseOptimizerConfig(
            kind=kind, lr=float(m.one("lr", 0.002)), eps=eps, weight_decay=float(m.one("weight_decay", 0.0)),
            gradient_clipping=bool(m.one("gradient_clipping", False)), max_gradient=float(m.one("max_gradient", 1.0)),
            rho=float(m.one("rho", 0.95)), alpha=float(m.one("alpha", 0.99)),
        )
    for key, kind in table.items():
        if opt.has(key):
            m = opt.one(key)
            return SparseOptimizerConfig(
                kind=kind, lr=float(m.one("lr", 0.002)), weight_decay=float(m.one("weight_decay", 0.0)),
                weight_decay_mode=str(m.one("weight_decay_mode", "NONE")).lower(),
                gradient_clipping=bool(m.one("gradient_clipping", False)),
                max_gradient=float(m.one("max_gradient", 1.0)),
                initial_accumulator_value=float(m.one("initial_accumulator_value", 0.0)),
                beta1=float(m.one("beta1", 0.9)), beta2=float(m.one("beta2", 0.999)),
                momentum=float(m.one("momentum", 0.9)),
            )
    raise ValueError(f"Unknown optimizer: {[k for k in opt.keys()]}")


def dense_optimizer_from_config(opt: Msg) -> DenseOptimizerConfig:
    """create_dense_optimizer / create_part_optimizer (tzrec/optim/optimizer_builder.py:100-151): the member of the `optimizer`
    oneof with every field of its message, defaults from protos/optimizer.proto:159-208, and the same for each of the
    block's `part_optimizers`.  `fields` keeps the config's names (beta1, beta2); `fused` selects torch's implementation and
    is dropped; `amsgrad: true` and fields the message does not have are refused by name."""
    members = [k for k in opt.keys() if k.endswith("_optimizer")]
    known = [k for k in members if k[:-len("_optimizer")] in DENSE_KINDS]
    if len(known) != 1 or len(members) != 1:
        raise ValueError(f"Unknown optimizer: {members[0] if len(members) == 1 else (members or None)}")
    kind = known[0][:-len("_optimizer")]
    given = {f: v[-1] for f, v in opt.one(known[0]).items()}
    group_options(kind, given)  # (refusals)
    fields = {f: (type(d)(given[f]) if f in given and not isinstance(d, bool) else given.get(f, d)) for f, d in DENSE_KINDS[kind].fields.items()}
    fields.pop("amsgrad", None)
    cfg = DenseOptimizerConfig(kind=kind, fields=fields, learning_rate=opt)
    if opt.has("regex_pattern"):
        cfg.regex_pattern = str(opt.one("regex_pattern"))
    for part in opt.many("part_optimizers"):
        sub = dense_optimizer_from_config(part)
        if sub.regex_pattern is None:
            raise ValueError("part_optimizers: regex_pattern is required")
        cfg.parts.append(sub)
    return cfg


def _sequence_blocks(g: Msg, seen_seq_names: List[str]):
    """The `sequence_groups` / `sequence_encoders` of one feature group, supplemented and validated as the reference's
    EmbeddingGroup._inspect_and_supplement_feature_group does (tzrec/modules/embedding.py:313-383): a single unnamed sequence
    group takes the parent's name, an encoder without `input` the only group; the parent's `embedding_name_suffix` is
    inherited (:240-250)."""
    name = g.one("group_name")
    sgs, encs = g.many("sequence_groups"), g.many("sequence_encoders")
    if not sgs and not encs:
        return [], []
    if str(g.one("group_type", "DEEP")) != "DEEP":
        raise ValueError(f"feature group {name}: sequence_groups and sequence_encoders belong in a DEEP group, this one is "
                         f"{g.one('group_type')}")
    if not encs:
        raise ValueError(f"feature group {name} has sequence_groups but no sequence_encoders")
    if not sgs:
        raise ValueError(f"feature group {name} has sequence_encoders but no sequence_groups")
    if len(sgs) > 1 and not all(sg.has("group_name") for sg in sgs):
        raise ValueError(f"feature group {name} has {len(sgs)} sequence_groups: every one of them needs a group_name")
    groups = []
    for sg in sgs:
        sname = str(sg.one("group_name", name))
        if sname in seen_seq_names:
            raise ValueError(f"sequence group name {sname} is used twice")
        seen_seq_names.append(sname)
        groups.append(SeqGroupSpec(sname, [str(f) for f in sg.many("feature_names")],
                                   sg.one("embedding_name_suffix") or g.one("embedding_name_suffix")))
    has_encoder = {sg.group_name: False for sg in groups}
    encoders = []
    for enc in encs:
        if len(enc) != 1:
            raise ValueError(f"feature group {name}: a sequence_encoders entry holds exactly one encoder, got {sorted(enc)}")
        (kind, body), = enc.items()
        if kind not in SEQ_ENCODER_KINDS:
            raise NotImplementedError(f"feature group {name}: sequence encoder {kind!r} is not built (built: {', '.join(SEQ_ENCODER_KINDS)})")
        m = body[-1]
        inp = m.one("input")
        if inp is None:
            if len(groups) != 1:
                raise ValueError(f"feature group {name} has {len(groups)} sequence_groups: its {kind} needs an `input`")
            inp = groups[0].group_name
        if inp not in has_encoder:
            raise ValueError(f"feature group {name}: {kind} reads {inp!r}, which is none of its sequence_groups {sorted(has_encoder)}")
        has_encoder[inp] = True
        spec = SeqEncoderSpec(kind=kind, input=str(inp), max_seq_length=int(m.one("max_seq_length", 0)))
        if kind == "din_encoder":
            if not m.has("attn_mlp"):
                raise ValueError(f"feature group {name}: din_encoder needs attn_mlp")
            other = sorted(k for k in m.one("attn_mlp") if k != "hidden_units")
            if other:  # (DINEncoder's attention MLP is the plain Linear + ReLU stack: nothing is dropped silently)
                raise NotImplementedError(f"feature group {name}: din_encoder attn_mlp fields {other}")
            spec.attn_mlp = {"hidden_units": [int(x) for x in m.one("attn_mlp").many("hidden_units")]}
        if kind == "pooling_encoder":
            spec.pooling_type = str(m.one("pooling_type", "mean"))
            if spec.pooling_type not in ("sum", "mean"):
                raise ValueError(f"feature group {name}: pooling_encoder pooling_type {spec.pooling_type!r}: sum | mean")
        encoders.append(spec)
    for sname, ok in has_encoder.items():
        if not ok:
            raise ValueError(f"feature group {name}: sequence group {sname} has no sequence encoder")
    return groups, encoders


def load_pipeline_spec(text: str) -> PipelineSpec:
    cfg = parse_text_proto(text)
    spec = PipelineSpec()
    def one_feature(kind: str, f: Msg, prefix: str = "", seq_len: int = 0) -> FeatureSpec:
        name = prefix + (f.one("feature_name") or f.one("sequence_name"))
        seq = dict(is_sequence=bool(prefix), sequence_length=seq_len)
        if kind == "id_feature":
            return FeatureSpec(
                name=name, kind=kind, is_sparse=True, embedding_dim=int(f.one("embedding_dim", 0)),
                num_embeddings=_num_embeddings(f, name), embedding_name=f.one("embedding_name"),
                pooling=str(f.one("pooling", "sum")).lower(), trainable=bool(f.one("trainable", True)),
                data_type=str(f.one("data_type", "FP32")).upper(),
                # id_feature.value_dim (tzrec/features/id_feature.py:42-50): configured, else 1 for a
                # sequence sub-feature (single id per step) and 0 = "any number of ids" otherwise
                value_dim=int(f.one("value_dim", 1 if prefix else 0)),
                zch=f.one("zch") if f.has("zch") else None, **seq)
        if kind == "raw_feature":
            nb = len(f.many("boundaries"))
            if nb:  # bucketized raw feature = a sparse id in [0, len(boundaries)]  (raw_feature.py:50-60)
                return FeatureSpec(name=name, kind=kind, is_sparse=True, embedding_dim=int(f.one("embedding_dim", 0)),
                                   num_embeddings=nb + 1, embedding_name=f.one("embedding_name"), **seq)
            return FeatureSpec(name=name, kind=kind, is_sparse=False, value_dim=int(f.one("value_dim", 1)), **seq)
        return FeatureSpec(name=name, kind=kind, is_sparse=f.has("embedding_dim"), embedding_dim=int(f.one("embedding_dim", 0)), **seq)

    _one_feature = one_feature

    def one_feature(kind: str, f: Msg, prefix: str = "", seq_len: int = 0) -> FeatureSpec:  # noqa: F811
        fs = _one_feature(kind, f, prefix, seq_len)
        if f.has("embedding_constraints"):
            fs.sharding_types = [str(t) for t in f.one("embedding_constraints").many("sharding_types")]
        return fs

    for fc in cfg.many("feature_configs"):
        (kind, body), = fc.items()
        f = body[-1]
        if kind == "sequence_feature":  # sub-features are named <sequence_name>__<feature_name> (feature.py)
            sname, slen = f.one("sequence_name"), int(f.one("sequence_length", 0))
            for sub in f.many("features"):
                (skind, sbody), = sub.items()
                spec.features.append(one_feature(skind, sbody[-1], prefix=f"{sname}__", seq_len=slen))
        else:
            spec.features.append(one_feature(kind, f))
    mc = cfg.one("model_config", Msg())
    seq_names: List[str] = []
    for g in mc.many("feature_groups"):
        seq_groups, seq_encoders = _sequence_blocks(g, seq_names)
        spec.feature_groups.append(FeatureGroupSpec(
            group_name=g.one("group_name"), feature_names=list(g.many("feature_names")),
            group_type=str(g.one("group_type", "DEEP")), embedding_name_suffix=g.one("embedding_name_suffix"),
            sequence_groups=seq_groups, sequence_encoders=seq_encoders))
    skip = {"feature_groups", "metrics", "losses", "num_class", "train_metrics", "variational_dropout",
            "kd", "use_pareto_loss_weight", "pareto"}
    for k, v in mc.items():
        if k not in skip and isinstance(v[-1], Msg):
            spec.model_name, spec.model = k, v[-1]
    spec.num_class = int(mc.one("num_class", 1))
    # (0 = the embedding group's fallback of 4, DeepFM's proto default; the xdeepfm message defaults to 16, rank_model.proto:69)
    spec.wide_embedding_dim = int(spec.model.one("wide_embedding_dim", 16 if spec.model_name == "xdeepfm" else 0)) if spec.model else 0
    tc = cfg.one("train_config", Msg())
    if tc.has("sparse_optimizer"):
        spec.sparse_optimizer = sparse_optimizer_from_config(tc.one("sparse_optimizer"))
        spec.sparse_optimizer_block = tc.one("sparse_optimizer")
    if tc.has("dense_optimizer"):
        spec.dense_optimizer_block = tc.one("dense_optimizer")
        spec.dense_optimizer = dense_optimizer_from_config(spec.dense_optimizer_block)
        for _, v in tc.one("dense_optimizer").items():
            if isinstance(v[-1], Msg) and v[-1].has("lr"):
                spec.dense_lr = float(v[-1].one("lr"))
    spec.gradient_accumulation_steps = int(tc.one("gradient_accumulation_steps", 0))
    if tc.has("grad_clipping"):
        from .optimizer import grad_clipping_from_msg

        spec.grad_clipping = grad_clipping_from_msg(tc.one("grad_clipping"))
    if tc.has("global_embedding_constraints"):
        spec.global_sharding_types = [str(t) for t in tc.one("global_embedding_constraints").many("sharding_types")]
    if tc.has("delta_embedding_dump_config"):  # enable_delta_embedding_dump, tzrec/main.py:691
        # the block stays tzrec's to interpret (its DeltaEmbeddingDumper owns cadence / files); its presence
        # is what asks the model for a ModelDeltaTracker (delta_embedding_dump.py)
        spec.delta_embedding_dump_config = tc.one("delta_embedding_dump_config")
    dc = cfg.one("data_config", Msg())
    spec.batch_size = int(dc.one("batch_size", 0))
    spec.label_fields = list(dc.many("label_fields"))
    spec.metrics = _metric_specs(mc.many("metrics"), None, spec.label_fields[0] if spec.label_fields else "label")
    for t in (spec.model.many("task_towers") if spec.model else []):
        spec.metrics += _metric_specs(t.many("metrics"), str(t.one("tower_name")), str(t.one("label_name")))
    spec.sample_weight_fields = [str(x) for x in dc.many("sample_weight_fields")]
    spec.sampler_kinds = [k for k in SAMPLER_KINDS if dc.has(k)]
    spec.model_config_keys = [str(k) for k in mc]
    if dc.has("negative_sampler"):
        ns = dc.one("negative_sampler")
        spec.negative_sampler = {**{k: v[-1] for k, v in ns.items()}, "num_sample": int(ns.one("num_sample", 0)),
                                 "attr_fields": [str(x) for x in ns.many("attr_fields")]}
    sparse_names = {f.name for f in spec.features if f.is_sparse}
    towers = spec.model.many("task_towers") if spec.model else []
    if mc.has("losses") or not towers:  # (a multi-task model reads its towers' blocks only, multi_task_rank.py:80-95)
        spec.losses = _loss_specs(mc.many("losses"), None, spec.num_class, sparse_names, match=spec.model_name in MATCH_MODELS)
    for t in towers:
        ts = TowerSpec(tower_name=str(t.one("tower_name")), label_name=str(t.one("label_name")), num_class=int(t.one("num_class", 1)),
                       weight=float(t.one("weight", 1.0)), sample_weight_name=t.one("sample_weight_name"),
                       task_space_indicator_label=t.one("task_space_indicator_label"),
                       in_task_space_weight=float(t.one("in_task_space_weight", 1.0)),
                       out_task_space_weight=float(t.one("out_task_space_weight", 1.0)))
        spec.task_towers.append(ts)
        spec.losses += _loss_specs(t.many("losses"), ts.tower_name, ts.num_class, sparse_names)
    return spec
