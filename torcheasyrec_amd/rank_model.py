"""Config-driven DLRM / DeepFM on top of EmbeddingGroup (the reference's model API surface).

`build_rank_model(spec)` takes what `config.load_pipeline_spec` read from a tzrec pipeline config
and builds the model the reference would build from the same file
(/root/reference/tzrec/main.py:134-166 picks the class from the model_config oneof;
/root/reference/tzrec/models/dlrm.py:26-135, deepfm.py:26-108, rank_model.py:83-262).
`forward(batch) -> {"logits", "probs"}`; `loss(predictions, batch) -> {"binary_cross_entropy": ...}`: one entry per
`losses { ... }` block of the config, keyed kind + tower suffix, each a fused call of losses.py (csrc/loss_ops.hip).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from . import _lib
from .config import PipelineSpec
from .dlrm import MLP, OutputLinear
from .embedding import SparseOptimizerConfig
from .embedding_group import Batch, EmbeddingGroup
from .interaction import CIN, Cross, CrossV2, FactorizationMachine, dot_interaction
from .losses import build_losses, output_to_prediction
from .masknet import MaskNetModule


def mlp_kwargs(msg) -> Dict[str, object]:
    """An MLP proto block (tzrec/protos/module.proto:4-17: hidden_units, dropout_ratio, activation,
    use_bn, bias, use_ln) as the module's keyword arguments (the reference's config_to_kwargs)."""
    return {"hidden_units": [int(x) for x in msg.many("hidden_units")], "bias": bool(msg.one("bias", True)),
            "activation": str(msg.one("activation", "nn.ReLU")), "use_bn": bool(msg.one("use_bn", False)),
            "dropout_ratio": [float(x) for x in msg.many("dropout_ratio")], "use_ln": bool(msg.one("use_ln", False))}


def mlp_from_msg(in_features: int, msg) -> MLP:
    """Every tower of the config-built models goes through here: no MLP field is dropped silently."""
    return MLP(in_features, **mlp_kwargs(msg))


class RankModel(nn.Module):
    # set by build_rank_model(..., process_group=...): tables sharded over the group's ranks, dense
    # parameters data-parallel (the DistributedModelParallel seam, tzrec/main.py:783-804)
    _build_pg = None
    _build_plan = None
    _build_use_planner = False
    _build_exchange = "exact"

    def __init__(self, spec: PipelineSpec, device: Optional[torch.device], sparse_optimizer: Optional[SparseOptimizerConfig]) -> None:
        super().__init__()
        self._spec = spec
        self._label = spec.label_fields[0] if spec.label_fields else "label"
        self._pg = RankModel._build_pg
        self._losses = build_losses(spec)  # (refusals and validation happened when the spec was built)
        self._model_losses = [l for l in self._losses if l.tower is None]
        self.embedding_group = EmbeddingGroup(
            spec.features, spec.feature_groups, wide_embedding_dim=spec.wide_embedding_dim or None,
            device=device, sparse_optimizer=sparse_optimizer if sparse_optimizer is not None else spec.sparse_optimizer,
            process_group=self._pg, plan=RankModel._build_plan,
            global_sharding_types=getattr(spec, "global_sharding_types", ()), batch_size=spec.batch_size or 1024,
            use_planner=RankModel._build_use_planner, exchange=RankModel._build_exchange)

    def sync_dense_parameters(self) -> None:
        """Same dense parameters on every rank (DDP broadcasts rank 0's at construction)."""
        if self._pg is not None:
            import torch.distributed as dist

            from .sharding import stream_collective

            for p in self.dense_parameters():
                stream_collective(dist.broadcast, p.data, src=0, group=self._pg)

    def allreduce_dense_grads(self) -> None:
        """DDP semantics for the dense parameters: average their gradients over the ranks (one flat
        all-reduce); sparse gradients were already applied by the owners inside backward."""
        if self._pg is None:
            return
        from .sharding import allreduce_average

        allreduce_average([p.grad for p in self.dense_parameters() if p.grad is not None], self._pg)

    def build_input(self, batch: Batch) -> Dict[str, torch.Tensor]:
        return self.embedding_group(batch)

    def dense_parameters(self):
        for n, p in self.named_parameters():
            # (the sequence encoders of a DEEP group live inside the embedding group, as in the reference: dense all the same)
            if not n.startswith("embedding_group.") or n.startswith("embedding_group._group_name_to_seq_encoders."):
                yield p

    @property
    def fused_optimizer(self):
        return self.embedding_group.fused_optimizer

    def _output_to_prediction(self, y: torch.Tensor) -> Dict[str, torch.Tensor]:
        return output_to_prediction(y, [l.spec for l in self._model_losses], self._spec.num_class)  # rank_model.py:133-179

    def loss(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        out = {}
        for l in self._model_losses:
            if l.plain_bce:  # mean BCE and nothing else: torch's, as before the `losses` block was read
                label = batch.labels[self._label].to(torch.float32)
                out[l.name] = nn.functional.binary_cross_entropy_with_logits(predictions["logits"], label)
            else:
                out[l.name] = l(predictions, batch)
        return out


class ConfigDLRM(RankModel):
    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        names = eg.group_names()
        self._sparse_group = names[0] if len(names) == 1 else "sparse"
        self._dense_group = "dense"
        self.dense_mlp = None
        if len(names) > 1 and eg.has_group(self._dense_group):
            self.dense_mlp = mlp_from_msg(eg.group_total_dim(self._dense_group), m.one("dense_mlp"))
        dims = set(eg.group_dims(self._sparse_group))
        if len(dims) > 1:
            raise Exception(f"sparse group feature dims must be the same, but we find {dims}")
        self._dim = dims.pop()
        self._num_sparse = len(eg.group_dims(self._sparse_group))
        if self.dense_mlp and self._dim != self.dense_mlp.output_dim():
            raise Exception("dense mlp last hidden_unit must be the same sparse feature dim")
        self._arch_with_sparse = bool(m.one("arch_with_sparse", True))
        n = self._num_sparse + (1 if self.dense_mlp else 0)
        feat = n * (n - 1) // 2 + (self._dim if self.dense_mlp else 0) + (self._num_sparse * self._dim if self._arch_with_sparse else 0)
        self.final_mlp = mlp_from_msg(feat, m.one("final"))
        self.output_mlp = OutputLinear(self.final_mlp.output_dim(), spec.num_class)
        if device is not None:
            for mod in (self.dense_mlp, self.final_mlp, self.output_mlp):
                if mod is not None:
                    mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        g = self.build_input(batch)
        sparse = g[self._sparse_group]
        d = self.dense_mlp(g[self._dense_group]) if self.dense_mlp else None
        allf = dot_interaction(d, sparse, self._dim, cat_dense=True, cat_sparse=self._arch_with_sparse)
        return self._output_to_prediction(self.output_mlp(self.final_mlp(allf)))


class ConfigDeepFM(RankModel):
    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        self._has_fm = eg.has_group("fm")
        fm_dims = eg.group_dims("fm" if self._has_fm else "deep")
        assert len(set(fm_dims)) == 1, f"embedding dimension of fm features must be same. but got {set(fm_dims)}"
        self._fm_n, self._fm_dim = len(fm_dims), fm_dims[0]
        self.fm = FactorizationMachine()
        self.deep_mlp = mlp_from_msg(eg.group_total_dim("deep"), m.one("deep"))
        final_dim = self.deep_mlp.output_dim()
        self.final_mlp = None
        if m.has("final"):
            self.final_mlp = mlp_from_msg(1 + self._fm_dim + final_dim, m.one("final"))
            final_dim = self.final_mlp.output_dim()
        self.output_mlp = OutputLinear(final_dim, spec.num_class)
        if device is not None:
            for mod in (self.deep_mlp, self.final_mlp, self.output_mlp):
                if mod is not None:
                    mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        g = self.build_input(batch)
        y_wide = torch.sum(g["wide"], dim=1, keepdim=True)
        y_deep = self.deep_mlp(g["deep"])
        fm_feat = (g["fm"] if self._has_fm else g["deep"]).reshape(-1, self._fm_n, self._fm_dim)
        y_fm = self.fm(fm_feat)
        if self.final_mlp is not None:
            y = self.output_mlp(self.final_mlp(torch.cat([y_wide, y_fm, y_deep], dim=1)))
        else:
            y = y_wide + torch.sum(y_fm, dim=1, keepdim=True) + self.output_mlp(y_deep)
        return self._output_to_prediction(y)


JAGGED_DIN = True  # multi_tower_din: DIN towers on the jagged positions (False: the reference's padded tensors)


class ConfigMultiTowerDIN(RankModel):
    """`multi_tower_din {...}` (tzrec/models/multi_tower_din.py:36-111): one MLP tower per DEEP group,
    one DIN target-attention tower per SEQUENCE group, concatenated, optional final MLP, logits layer."""

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        from .sequence import DIN_JAGGED_MAX_LEN, DINEncoder

        eg, m = self.embedding_group, spec.model
        self.towers = nn.ModuleDict()
        total = 0
        for tower in m.many("towers"):
            g = str(tower.one("input"))
            mlp = mlp_from_msg(eg.group_total_dim(g), tower.one("mlp"))
            self.towers[g] = mlp
            total += mlp.output_dim()
        self.din_towers = nn.ModuleList()
        for tower in m.many("din_towers"):
            g = str(tower.one("input"))
            din = DINEncoder(eg.group_total_dim(f"{g}.sequence"), eg.group_total_dim(f"{g}.query"), g,
                             attn_mlp={"hidden_units": [int(x) for x in tower.one("attn_mlp").many("hidden_units")]})
            self.din_towers.append(din)
            total += din.output_dim()
            # the tower takes the group's sequences as rows of the unpooled lookup (no padding) when its attention MLP is
            # the plain Linear + ReLU stack and the group's sequence features come from ONE sequence_feature block (one
            # set of lengths): csrc/din_attention.hip
            info = eg._seq_info.get(g) if hasattr(eg, "_seq_info") else None
            if JAGGED_DIN and info is not None and din.jagged_capable() and len({f.name.split("__")[0] for f in info["sequence"]}) == 1 \
                    and not any(getattr(f, "value_dim", 1) not in (0, 1) for f in info["sequence"]) \
                    and info.get("max_len") and int(info["max_len"]) <= DIN_JAGGED_MAX_LEN:
                # (a group without a configured sequence_length pads to the batch's longest sequence in the reference: nothing
                # is truncated there, and the jagged kernels keep at most DIN_JAGGED_MAX_LEN positions of a sample -- such
                # groups stay on the padded form)
                if g not in eg.nested_sequence_groups() or g in eg.jagged_sequence_groups:  # (a nested group: only with its encoders)
                    eg.jagged_sequence_groups.add(g)
            else:
                eg.jagged_sequence_groups.discard(g)  # (a nested group of a DEEP group: this tower reads its padded tensor)
        self.final_mlp = None
        if m.has("final"):
            self.final_mlp = mlp_from_msg(total, m.one("final"))
            total = self.final_mlp.output_dim()
        self.output_mlp = OutputLinear(total, spec.num_class)
        if device is not None:
            for mod in (self.towers, self.din_towers, self.final_mlp, self.output_mlp):
                if mod is not None:
                    mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        g = self.build_input(batch)
        outs = [mlp(g[name]) for name, mlp in self.towers.items()]
        outs += [din(g) for din in self.din_towers]
        y = torch.cat(outs, dim=-1)
        if self.final_mlp is not None:
            y = self.final_mlp(y)
        return self._output_to_prediction(self.output_mlp(y))


FUSED_MOE_MIX = True  # A/B switch: False = the reference's stack / softmax / batched-matmul form


class MMoE(nn.Module):
    """Multi-gate mixture of experts, the reference module's constructor and forward
    (tzrec/modules/mmoe.py:20-76): `num_expert` expert MLPs over the input, per task an optional
    gate MLP and a Linear + softmax over the experts; returns one mixed tensor per task."""

    def __init__(self, in_features: int, expert_mlp: Dict[str, object], num_expert: int, num_task: int,
                 gate_mlp: Optional[Dict[str, object]] = None) -> None:
        super().__init__()
        self.num_expert, self.num_task = num_expert, num_task
        self.expert_mlps = nn.ModuleList([MLP(in_features, **expert_mlp) for _ in range(num_expert)])
        gate_in = in_features
        self.has_gate_mlp = gate_mlp is not None
        if self.has_gate_mlp:
            self.gate_mlps = nn.ModuleList([MLP(in_features, **gate_mlp) for _ in range(num_task)])
            gate_in = self.gate_mlps[0].hidden_units[-1]
        self.gate_finals = nn.ModuleList([OutputLinear(gate_in, num_expert) for _ in range(num_task)])  # (nn.Linear's parameters; <= 8 units: one-pass kernels)

    def output_dim(self) -> int:
        return self.expert_mlps[0].hidden_units[-1]

    def forward(self, input: torch.Tensor):
        outs = [e(input) for e in self.expert_mlps]
        logits = [self.gate_finals[i](self.gate_mlps[i](input) if self.has_gate_mlp else input) for i in range(self.num_task)]
        if FUSED_MOE_MIX and input.dim() == 2 and (input.is_cuda or _lib.emulated()):
            from .gate_ops import moe_mix, moe_mix_ok

            if moe_mix_ok(logits, outs):  # softmax + mixing of every task in one launch per direction, nothing stacked (csrc/gate_mix.hip)
                return moe_mix(logits, outs)
        experts = torch.stack(outs, dim=1)  # [B, E, H]: the reference's literal form
        return [torch.matmul(torch.softmax(lg, dim=1).unsqueeze(1), experts).squeeze(1) for lg in logits]


class MultiTaskRankModel(RankModel):
    """What the multi-task models share (tzrec/models/multi_task_rank.py): a task tower (optional MLP + logits layer) per
    `task_towers` block; predictions and losses carry the tower name as suffix."""

    def _build_towers(self, m, in_dims, copies: int = 1) -> None:
        """`in_dims[i]`: width of the tensor the tower(s) of block i read; `copies` towers per block, block-major (pepnet: one per
        domain)"""
        self._towers = [(str(t.one("tower_name")), str(t.one("label_name"))) for t in m.many("task_towers")]
        self.task_mlps = nn.ModuleList()
        self.task_outputs = nn.ModuleList()
        self._tower_losses = [[l for l in self._losses if l.tower is not None and l.tower.tower_name == name] for name, _ in self._towers]
        for t, d_in in zip(m.many("task_towers"), in_dims):
            for _ in range(copies):
                d = d_in
                if t.has("mlp"):
                    self.task_mlps.append(mlp_from_msg(d, t.one("mlp")))
                    d = self.task_mlps[-1].output_dim()
                else:
                    self.task_mlps.append(nn.Identity())
                self.task_outputs.append(OutputLinear(d, int(t.one("num_class", 1))))

    def _tower_predictions(self, task_inputs) -> Dict[str, torch.Tensor]:
        out: Dict[str, torch.Tensor] = {}
        for i, (tower, _) in enumerate(self._towers):
            y = self.task_outputs[i](self.task_mlps[i](task_inputs[i]))
            out.update(output_to_prediction(y, [l.spec for l in self._tower_losses[i]], self.task_outputs[i].out_features, f"_{tower}"))
        return out

    def loss(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        from .dlrm import bce_with_logits

        out = {}
        for (tower, label), losses in zip(self._towers, self._tower_losses):
            for l in losses:
                if l.plain_bce:  # (tzr_bce_logits: the launches of before)
                    out[l.name] = bce_with_logits(predictions[f"logits_{tower}"], batch.labels[label])
                else:
                    out[l.name] = l(predictions, batch)
        return out


class ConfigMMoE(MultiTaskRankModel):
    """`mmoe {...}` (tzrec/models/mmoe.py:36-96): the MMoE module over the (single) feature group and
    a task tower (MLP + logits layer) per task.  Predictions and losses carry the tower name as
    suffix, as the reference's multi-task models do."""

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        self._group = eg.group_names()[0]
        d_in = eg.group_total_dim(self._group)
        expert = mlp_kwargs(m.one("expert_mlp"))
        hidden = expert["hidden_units"]
        gate = mlp_kwargs(m.one("gate_mlp")) if m.has("gate_mlp") else None
        n_task = len(m.many("task_towers"))
        self.mmoe = MMoE(d_in, expert, int(m.one("num_expert")), n_task, gate)
        self._build_towers(m, [hidden[-1]] * n_task)
        if device is not None:
            for mod in (self.mmoe, self.task_mlps, self.task_outputs):
                mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        return self._tower_predictions(self.mmoe(self.build_input(batch)[self._group]))


class ConfigPLE(MultiTaskRankModel):
    """`ple {...}` (tzrec/models/ple.py:27-109): stacked CGC levels (`extraction_networks`, ple.ExtractionNet) over the (single)
    feature group -- level 0 feeds it to every task's experts and to the shared ones, the last level has no shared gate -- and
    a task tower per task on the last level's task outputs.  Refused when built, by the level's name, what the reference
    itself cannot run: a level without shared experts (`share_num` absent or 0) or without task experts, a level without
    `share_expert_net` (the reference reads it unconditionally) or `task_expert_net`, task and shared experts of one level that
    end in different widths (its `torch.stack` fails on the first batch), a field the block does not have."""

    _LEVEL_FIELDS = ("network_name", "expert_num_per_task", "share_num", "task_expert_net", "share_expert_net")

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        from .ple import ExtractionNet

        eg, m = self.embedding_group, spec.model
        self._group = eg.group_names()[0]
        d_in = eg.group_total_dim(self._group)
        n_task = len(m.many("task_towers"))
        levels = m.many("extraction_networks")
        if not levels or n_task == 0:
            raise ValueError("ple: needs at least one `extraction_networks` block and one `task_towers` block")
        self._extraction_nets = nn.ModuleList()
        in_tasks, in_shared = [d_in] * n_task, d_in
        for i, lv in enumerate(levels):
            name = str(lv.one("network_name", f"level{i}"))
            other = sorted(k for k in lv if k not in self._LEVEL_FIELDS)
            if other:
                raise ValueError(f"ple: extraction_networks {name!r} has no field {other[0]!r} (fields: {', '.join(self._LEVEL_FIELDS)})")
            share_num, per_task = int(lv.one("share_num", 0)), int(lv.one("expert_num_per_task", 0))
            if share_num <= 0:
                raise ValueError(f"ple: extraction_networks {name!r} needs share_num >= 1 (the reference cannot run a level without shared experts)")
            if per_task <= 0:
                raise ValueError(f"ple: extraction_networks {name!r} needs expert_num_per_task >= 1")
            for blk in ("share_expert_net", "task_expert_net"):
                if not lv.has(blk):
                    raise ValueError(f"ple: extraction_networks {name!r} needs `{blk}`")
            share_net, task_net = mlp_kwargs(lv.one("share_expert_net")), mlp_kwargs(lv.one("task_expert_net"))
            if not share_net["hidden_units"] or not task_net["hidden_units"]:
                raise ValueError(f"ple: extraction_networks {name!r}: an expert net needs hidden_units")
            if share_net["hidden_units"][-1] != task_net["hidden_units"][-1]:
                raise ValueError(f"ple: extraction_networks {name!r}: task experts end {task_net['hidden_units'][-1]} wide, shared experts "
                                 f"{share_net['hidden_units'][-1]}: one gate mixes both, the widths must be equal")
            net = ExtractionNet(in_tasks, in_shared, name, share_num, per_task, share_net, task_net, final_flag=i == len(levels) - 1)
            self._extraction_nets.append(net)
            dims = net.output_dim()
            in_tasks, in_shared = dims[:-1], dims[-1]
        self._build_towers(m, in_tasks)
        if device is not None:
            for mod in (self._extraction_nets, self.task_mlps, self.task_outputs):
                mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        net = self.build_input(batch)[self._group]
        task_fea, shared_fea = [net] * len(self._towers), net
        for level in self._extraction_nets:
            task_fea, shared_fea = level(task_fea, shared_fea)
        return self._tower_predictions(task_fea)


class ConfigPEPNet(MultiTaskRankModel):
    """`pepnet {...}` (tzrec/models/pepnet.py:27-245): feature group `all` is the main embedding; with a group `domain` EPNet
    scales it by a gate over [domain | all.detach()]; with a group `uia` PPNet runs per task a gated stack over it
    (personalized_net.EPNet / PPNet, the gate-and-scale step of every level in one launch); a task tower per task on PPNet's
    output, or all towers on the EPNet output / the main embedding without it.

    With `domain_input_name` every task has `task_domain_num` towers, in the order task * D + domain; the predictions carry the
    keys `<kind>_<tower>_<domain>`, and loss and metrics read, per sample, the prediction of the domain
    `batch.labels[domain_input_name]` names (`select_domain_predictions`).  The selection is a mask-and-sum over the D
    predictions -- no gather, no device-side index check, capturable --, so a row whose id lies outside [0, D) selects nothing:
    every selected value of that row (logit and probability alike) is 0 and no tower receives a gradient from it.  (The
    reference's torch.gather faults on such a row.)

    Refused when built, naming the field, what the reference cannot run: no `all` group (feature_groups), a `uia` group with
    empty `ppnet_hidden_units`, a `ppnet_dropout_ratio` list whose length is neither 0, 1 nor that of `ppnet_hidden_units`,
    `task_domain_num` < 1, a `domain_input_name` that is no `data_config.label_fields` entry, a field the block does not have."""

    _FIELDS = ("epnet_hidden_unit", "epnet_gamma", "ppnet_hidden_units", "ppnet_activation", "ppnet_dropout_ratio", "ppnet_gamma",
               "domain_input_name", "task_domain_num", "task_towers")

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        from .personalized_net import EPNet, PPNet

        eg, m = self.embedding_group, spec.model
        other = sorted(k for k in m if k not in self._FIELDS)
        if other:
            raise ValueError(f"pepnet: pepnet has no field {other[0]!r} (fields: {', '.join(self._FIELDS)})")
        if not eg.has_group("all"):
            raise ValueError("pepnet: feature_groups needs a group named 'all' (the main embedding)")
        n_task = len(m.many("task_towers"))
        if n_task == 0:
            raise ValueError("pepnet: needs at least one `task_towers` block")
        main_dim = eg.group_total_dim("all")
        task_in = main_dim
        self.epnet = None
        if eg.has_group("domain"):
            self.epnet = EPNet(main_dim, eg.group_total_dim("domain"), hidden_dim=int(m.one("epnet_hidden_unit", main_dim)),
                               gamma=float(m.one("epnet_gamma", 2.0)))
            task_in = self.epnet.output_dim()
        self.ppnet = None
        if eg.has_group("uia"):
            hidden = [int(x) for x in m.many("ppnet_hidden_units")]
            drops = [float(x) for x in m.many("ppnet_dropout_ratio")]
            if not hidden:
                raise ValueError("pepnet: a 'uia' feature group needs ppnet_hidden_units (PPNet without a layer has no output)")
            if len(drops) not in (0, 1, len(hidden)):
                raise ValueError(f"pepnet: ppnet_dropout_ratio has {len(drops)} entries, ppnet_hidden_units {len(hidden)}: none, one or one per layer")
            self.ppnet = PPNet(main_dim, eg.group_total_dim("uia"), num_task=n_task, hidden_units=hidden,
                               activation=str(m.one("ppnet_activation", "nn.ReLU")), dropout_ratio=drops, gamma=float(m.one("ppnet_gamma", 2.0)))
            task_in = self.ppnet.task_output_dim()
        self._domain_input_name = str(m.one("domain_input_name")) if m.has("domain_input_name") else None
        self._task_domain_num = int(m.one("task_domain_num", 1))
        if self._task_domain_num < 1:
            raise ValueError(f"pepnet: task_domain_num is {self._task_domain_num}: at least 1")
        if self._domain_input_name is not None and self._domain_input_name not in spec.label_fields:
            raise ValueError(f"pepnet: domain_input_name {self._domain_input_name!r} is not one of data_config.label_fields "
                             f"({', '.join(spec.label_fields)}): the domain id of a sample is read from batch.labels")
        self._build_towers(m, [task_in] * n_task, copies=self._task_domain_num if self._domain_input_name else 1)
        if device is not None:
            for mod in (self.epnet, self.ppnet, self.task_mlps, self.task_outputs):
                if mod is not None:
                    mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        g = self.build_input(batch)
        feat = g["all"]
        if self.epnet is not None:
            feat = self.epnet(feat, g["domain"])
        n_task = len(self._towers)
        task_inputs = self.ppnet(feat, g["uia"]) if self.ppnet is not None else [feat] * n_task
        if self._domain_input_name is None:
            return self._tower_predictions(task_inputs)
        D = self._task_domain_num
        out: Dict[str, torch.Tensor] = {}
        for i, (tower, _) in enumerate(self._towers):
            for d in range(D):
                k = i * D + d
                y = self.task_outputs[k](self.task_mlps[k](task_inputs[i]))
                out.update(output_to_prediction(y, [l.spec for l in self._tower_losses[i]], self.task_outputs[k].out_features, f"_{tower}_{d}"))
        return out

    def select_domain_predictions(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        """`<kind>_<tower>`: per sample the `<kind>_<tower>_<d>` of d = batch.labels[domain_input_name] (the reference's
        _select_domain_task_output); a row with d outside [0, D) gets 0.  Without `domain_input_name`: the predictions as
        they are."""
        if self._domain_input_name is None:
            return predictions
        D = self._task_domain_num
        idx = batch.labels[self._domain_input_name].reshape(-1)
        masks = [idx == d for d in range(D)]
        out: Dict[str, torch.Tensor] = {}
        for tower, _ in self._towers:
            tail = f"_{tower}_0"
            for key in [k for k in predictions if k.endswith(tail)]:
                kind = key[:-len(tail)]
                vals = [predictions[f"{kind}_{tower}_{d}"] for d in range(D)]
                shape = (-1,) + (1,) * (vals[0].dim() - 1)
                sel = vals[0] * masks[0].to(vals[0].dtype).view(shape)
                for d in range(1, D):
                    sel = sel + vals[d] * masks[d].to(vals[d].dtype).view(shape)
                out[f"{kind}_{tower}"] = sel
        return out

    def loss(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        return super().loss(self.select_domain_predictions(predictions, batch), batch)


FUSED_RELATION_CHAIN = True  # A/B switch: False = the reference's literal cat / MLP form of DBMTL's relation towers


class ConfigDBMTL(MultiTaskRankModel):
    """`dbmtl {...}` (tzrec/models/dbmtl.py:28-175): over the (single, first) feature group an optional `mask_net`
    (masknet.MaskNetModule), an optional `bottom_mlp`, an optional MMoE (present iff `expert_mlp`; `num_expert` defaults to 3),
    then per `task_towers` block an optional `mlp`, an optional `relation_mlp` over [the tower's own output | the relation
    outputs of the towers `relation_tower_names` lists] and the logits layer.  A tower has a relation net only if it has
    `relation_mlp` (`relation_tower_names` without it is ignored; `relation_mlp` without names runs over the tower's own
    output); the relation output of a tower without one is its `mlp` output.  `task_mlps` and `relation_mlps` are ModuleDicts
    keyed by tower name, `task_outputs` a ModuleList, as in the reference.

    All relation MLPs of the model run in one launch forward and two backward (gate_ops.relation_chain, csrc/relation_chain.hip)
    with no concat tensor; the literal form runs with FUSED_RELATION_CHAIN off, with a relation MLP that is not plain Linear +
    bias + ReLU, with a shape outside the kernel's limits, or off the GPU / the emulator.

    Refused when built, naming tower and field, what the reference cannot run (it dies with a KeyError on the first batch): a
    `relation_tower_names` entry that stands later in the config, does not exist or is the tower itself; a duplicate
    `tower_name`; a field the block or a tower does not have.  `pareto_min_loss_weight` and `train_metrics` are refused by
    name: not built."""

    _FIELDS = ("mask_net", "bottom_mlp", "expert_mlp", "gate_mlp", "num_expert", "task_towers")
    _TOWER_FIELDS = ("tower_name", "label_name", "metrics", "losses", "num_class", "mlp", "weight", "relation_tower_names", "relation_mlp",
                     "sample_weight_name", "task_space_indicator_label", "in_task_space_weight", "out_task_space_weight")
    _MASK_FIELDS = ("n_mask_blocks", "mask_block", "top_mlp", "use_parallel")

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        other = sorted(k for k in m if k not in self._FIELDS)
        if other:
            raise ValueError(f"dbmtl: dbmtl has no field {other[0]!r} (fields: {', '.join(self._FIELDS)})")
        towers = m.many("task_towers")
        if not towers:
            raise ValueError("dbmtl: needs at least one `task_towers` block")
        names = []
        for t in towers:
            name = str(t.one("tower_name"))
            for k in ("pareto_min_loss_weight", "train_metrics"):
                if t.has(k):
                    raise NotImplementedError(f"dbmtl: task_towers {name!r}: `{k}` is not built")
            other = sorted(k for k in t if k not in self._TOWER_FIELDS)
            if other:
                raise ValueError(f"dbmtl: task_towers {name!r} has no field {other[0]!r} (fields: {', '.join(self._TOWER_FIELDS)})")
            if name in names:
                raise ValueError(f"dbmtl: tower_name {name!r} stands twice in task_towers")
            names.append(name)
        self._group = eg.group_names()[0]
        d = eg.group_total_dim(self._group)
        self.mask_net = None
        if m.has("mask_net"):
            mod = m.one("mask_net")
            other = sorted(k for k in mod if k not in self._MASK_FIELDS)
            if other:
                raise ValueError(f"dbmtl: mask_net has no field {other[0]!r} (fields: {', '.join(self._MASK_FIELDS)})")
            for k in ("n_mask_blocks", "mask_block"):
                if not mod.has(k):
                    raise ValueError(f"dbmtl: mask_net needs `{k}`")
            blk = mod.one("mask_block")
            if not blk.has("hidden_dim"):
                raise ValueError("dbmtl: mask_net.mask_block needs `hidden_dim`")
            mask_block = {"hidden_dim": int(blk.one("hidden_dim")), "reduction_ratio": float(blk.one("reduction_ratio", 1.0))}
            if blk.has("aggregation_dim"):
                mask_block["aggregation_dim"] = int(blk.one("aggregation_dim"))
            self.mask_net = MaskNetModule(d, int(mod.one("n_mask_blocks")), mask_block,
                                          top_mlp=mlp_kwargs(mod.one("top_mlp")) if mod.has("top_mlp") else None,
                                          use_parallel=bool(mod.one("use_parallel", True)))
            d = self.mask_net.output_dim()
        self.bottom_mlp = None
        if m.has("bottom_mlp"):
            self.bottom_mlp = mlp_from_msg(d, m.one("bottom_mlp"))
            d = self.bottom_mlp.output_dim()
        self.mmoe = None
        if m.has("expert_mlp"):
            self.mmoe = MMoE(d, mlp_kwargs(m.one("expert_mlp")), int(m.one("num_expert", 3)), len(towers),
                             mlp_kwargs(m.one("gate_mlp")) if m.has("gate_mlp") else None)
            d = self.mmoe.output_dim()
        self._build_bayes_towers(m, d)
        if device is not None:
            for mod in (self.mask_net, self.bottom_mlp, self.mmoe, self.task_mlps, self.relation_mlps, self.task_outputs):
                if mod is not None:
                    mod.to(device)

    def _build_bayes_towers(self, m, d_in: int) -> None:
        """task_mlps / relation_mlps by tower name, task_outputs by position (dbmtl.py:84-123); `_relations[i]`: the positions
        of the towers whose relation output tower i's relation MLP reads"""
        towers = m.many("task_towers")
        self._towers = [(str(t.one("tower_name")), str(t.one("label_name"))) for t in towers]
        self._tower_losses = [[l for l in self._losses if l.tower is not None and l.tower.tower_name == name] for name, _ in self._towers]
        names = [name for name, _ in self._towers]
        self.task_mlps = nn.ModuleDict()
        self.relation_mlps = nn.ModuleDict()
        self.task_outputs = nn.ModuleList()
        self._relations = []
        widths = []  # of every tower's relation output
        for i, t in enumerate(towers):
            name, d = names[i], d_in
            if t.has("mlp"):
                self.task_mlps[name] = mlp_from_msg(d, t.one("mlp"))
                d = self.task_mlps[name].output_dim()
            rel = []
            if t.has("relation_mlp"):
                for r in (str(x) for x in t.many("relation_tower_names")):
                    if r == name:
                        raise ValueError(f"dbmtl: task_towers {name!r}: relation_tower_names names the tower itself")
                    if r not in names:
                        raise ValueError(f"dbmtl: task_towers {name!r}: relation_tower_names entry {r!r} is no tower_name ({', '.join(names)})")
                    if names.index(r) > i:
                        raise ValueError(f"dbmtl: task_towers {name!r}: relation_tower_names entry {r!r} stands later in the config; "
                                         "a relation MLP reads towers before it")
                    rel.append(names.index(r))
                self.relation_mlps[name] = mlp_from_msg(d + sum(widths[j] for j in rel), t.one("relation_mlp"))
                d = self.relation_mlps[name].output_dim()
            self._relations.append(rel)
            widths.append(d)
            self.task_outputs.append(OutputLinear(d, int(t.one("num_class", 1))))

    def _relation_outputs(self, task_net):
        """the relation output of every tower (dbmtl.py:155-167)"""
        names = [name for name, _ in self._towers]
        mlps = [self.relation_mlps[n] if n in self.relation_mlps else None for n in names]
        x0 = task_net[0]
        if FUSED_RELATION_CHAIN and any(m is not None for m in mlps) and x0.dim() == 2 and (x0.is_cuda or _lib.emulated()) \
                and all(m is None or m._plain for m in mlps):
            from .gate_ops import relation_chain, relation_chain_ok

            xs = [_lib.rows16(x) for x in task_net]
            for i in range(len(xs)):  # (towers that read one tensor: one object, as they came)
                for j in range(i):
                    if task_net[i] is task_net[j]:
                        xs[i] = xs[j]
            layers = [[] if m is None else [(lin.weight, lin.bias) for lin in m.linears()] for m in mlps]
            if relation_chain_ok(xs, self._relations, layers):  # every relation MLP of the model in one launch, no concat tensor
                return relation_chain(xs, self._relations, layers)
        out = []
        for i, m in enumerate(mlps):
            out.append(task_net[i] if m is None else m(torch.cat([task_net[i]] + [out[j] for j in self._relations[i]], dim=1)))
        return out

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        net = self.build_input(batch)[self._group]
        if self.mask_net is not None:
            net = self.mask_net(net)
        if self.bottom_mlp is not None:
            net = self.bottom_mlp(net)
        task_in = self.mmoe(net) if self.mmoe is not None else [net] * len(self._towers)
        task_net = [self.task_mlps[name](task_in[i]) if name in self.task_mlps else task_in[i] for i, (name, _) in enumerate(self._towers)]
        out: Dict[str, torch.Tensor] = {}
        for i, r in enumerate(self._relation_outputs(task_net)):
            tower = self._towers[i][0]
            out.update(output_to_prediction(self.task_outputs[i](r), [l.spec for l in self._tower_losses[i]], self.task_outputs[i].out_features,
                                            f"_{tower}"))
        return out


class ConfigDCNV1(RankModel):
    """`dcn_v1 {...}` (tzrec/models/dcn.py:36-73): the cross network and a deep MLP over the (single) feature group, a final MLP
    over [cross | deep], a logits layer without bias.  `cross { cross_num }` (protos/module.proto:82-85) defaults to 3 layers."""

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        self._group = eg.group_names()[0]
        d_in = eg.group_total_dim(self._group)
        cross = m.one("cross") if m.has("cross") else {}
        other = sorted(k for k in cross if k != "cross_num")
        if other:
            raise ValueError(f"dcn_v1: cross has no field {other[0]!r} (fields: cross_num)")
        self.cross = Cross(d_in, cross_num=int(cross.one("cross_num", 3)) if cross else 3)
        self.deep = mlp_from_msg(d_in, m.one("deep"))
        self.final_dnn = mlp_from_msg(self.cross.output_dim() + self.deep.output_dim(), m.one("final"))
        self.output_linear = OutputLinear(self.final_dnn.output_dim(), spec.num_class, bias=False)
        if device is not None:
            for mod in (self.cross, self.deep, self.final_dnn, self.output_linear):
                mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        features = self.build_input(batch)[self._group]
        y = torch.cat([self.cross(features), self.deep(features)], dim=-1)
        return self._output_to_prediction(self.output_linear(self.final_dnn(y)))


class ConfigDCNV2(RankModel):
    """`dcn_v2 {...}` (tzrec/models/dcn_v2.py:26-88): an optional `backbone` MLP over the (single) feature group, the low-rank
    cross network over its output (over the group itself without one), an optional `deep` MLP over the group whose output goes
    behind the cross output, a `final` MLP, a logits layer without bias.  `cross { cross_num low_rank }`
    (protos/module.proto:87-92) is required and defaults to 3 layers of rank 32."""

    _FIELDS = {"dcn_v2": ("backbone", "cross", "deep", "final"), "cross": ("cross_num", "low_rank")}

    @classmethod
    def _block(cls, parent, where: str, name: str, required: bool = True):
        other = sorted(k for k in parent if k not in cls._FIELDS[where])
        if other:
            raise ValueError(f"dcn_v2: {where} has no field {other[0]!r} (fields: {', '.join(cls._FIELDS[where])})")
        if not parent.has(name):
            if required:
                raise ValueError(f"dcn_v2: {where} needs `{name}`")
            return None
        return parent.one(name)

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        self._group = eg.group_names()[0]
        d_in = eg.group_total_dim(self._group)
        cross = self._block(m, "dcn_v2", "cross")
        final = self._block(m, "dcn_v2", "final")
        self._block(cross, "cross", "cross_num", required=False)  # (the block's own fields, by name)
        backbone, deep = self._block(m, "dcn_v2", "backbone", required=False), self._block(m, "dcn_v2", "deep", required=False)
        self.backbone = mlp_from_msg(d_in, backbone) if backbone is not None else None
        self.cross = CrossV2(self.backbone.output_dim() if self.backbone is not None else d_in,
                             cross_num=int(cross.one("cross_num", 3)), low_rank=int(cross.one("low_rank", 32)))
        self.deep = mlp_from_msg(d_in, deep) if deep is not None else None
        self.final_dnn = mlp_from_msg(self.cross.output_dim() + (self.deep.output_dim() if self.deep is not None else 0), final)
        self.output_linear = OutputLinear(self.final_dnn.output_dim(), spec.num_class, bias=False)
        if device is not None:
            for mod in (self.backbone, self.cross, self.deep, self.final_dnn, self.output_linear):
                if mod is not None:
                    mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        features = self.build_input(batch)[self._group]
        net = self.cross(self.backbone(features) if self.backbone is not None else features)
        if self.deep is not None:
            net = torch.cat([net, self.deep(features)], dim=-1)
        return self._output_to_prediction(self.output_linear(self.final_dnn(net)))


class ConfigXDeepFM(RankModel):
    """`xdeepfm {...}` (tzrec/models/xdeepfm.py:44-86): the compressed interaction network over the WIDE group, reshaped to
    [B, F, wide_embedding_dim] (16 when the config omits it, protos/models/rank_model.proto:69), a deep MLP over group `deep`,
    a final MLP over [cin | deep], a logits layer with bias.  `cin { cin_layer_size }` (protos/module.proto) is required."""

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        if not m.has("cin"):
            raise ValueError("xdeepfm: the model needs a `cin { cin_layer_size: ... }` block")
        cin = m.one("cin")
        other = sorted(k for k in cin if k != "cin_layer_size")
        if other:
            raise ValueError(f"xdeepfm: cin has no field {other[0]!r} (fields: cin_layer_size)")
        layers = [int(v) for v in cin.many("cin_layer_size")]
        if not layers:
            raise ValueError("xdeepfm: cin needs at least one cin_layer_size")
        wide_dims = eg.group_dims("wide")
        self._feature_num, self._wide_dim = len(wide_dims), spec.wide_embedding_dim
        assert set(wide_dims) == {self._wide_dim}, f"wide features must all have dim {self._wide_dim}, got {set(wide_dims)}"
        self.deep = mlp_from_msg(eg.group_total_dim("deep"), m.one("deep"))
        self.cin = CIN(self._feature_num, layers)
        self.final = mlp_from_msg(self.cin.output_dim() + self.deep.output_dim(), m.one("final"))
        self.output_mlp = OutputLinear(self.final.output_dim(), spec.num_class)
        if device is not None:
            for mod in (self.deep, self.cin, self.final, self.output_mlp):
                mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        g = self.build_input(batch)
        cin_feat = self.cin(g["wide"].reshape(-1, self._feature_num, self._wide_dim))
        y = self.final(torch.cat([cin_feat, self.deep(g["deep"])], dim=1))
        return self._output_to_prediction(self.output_mlp(y))


class ConfigMaskNet(RankModel):
    """`mask_net {...}` (tzrec/models/masknet.py:25-65): the MaskNet module over the (single) feature group, a logits layer
    without bias over `top_mlp.hidden_units[-1]`.  `mask_net_module { n_mask_blocks mask_block { reduction_ratio aggregation_dim
    hidden_dim } top_mlp {...} use_parallel }` (protos/module.proto:62-80): `reduction_ratio` defaults to 1.0 and
    `use_parallel` to true; `top_mlp` is optional in the proto, but the reference's model indexes its last hidden unit."""

    _FIELDS = {"mask_net": ("mask_net_module",), "mask_net_module": ("n_mask_blocks", "mask_block", "top_mlp", "use_parallel"),
               "mask_block": ("reduction_ratio", "aggregation_dim", "hidden_dim")}

    @classmethod
    def _block(cls, parent, where: str, name: str):
        other = sorted(k for k in parent if k not in cls._FIELDS[where])
        if other:
            raise ValueError(f"mask_net: {where} has no field {other[0]!r} (fields: {', '.join(cls._FIELDS[where])})")
        if not parent.has(name):
            raise ValueError(f"mask_net: {where} needs `{name}`")
        return parent.one(name)

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg = self.embedding_group
        self._group = eg.group_names()[0]
        mod = self._block(spec.model, "mask_net", "mask_net_module")
        n_blocks = self._block(mod, "mask_net_module", "n_mask_blocks")
        blk = self._block(mod, "mask_net_module", "mask_block")
        hidden_dim = self._block(blk, "mask_block", "hidden_dim")
        if not mod.has("top_mlp") or not mod.one("top_mlp").many("hidden_units"):
            raise ValueError("mask_net: mask_net_module needs `top_mlp { hidden_units: ... }` (the logits layer reads its last width)")
        mask_block = {"hidden_dim": int(hidden_dim), "reduction_ratio": float(blk.one("reduction_ratio", 1.0))}
        if blk.has("aggregation_dim"):
            mask_block["aggregation_dim"] = int(blk.one("aggregation_dim"))
        top = mlp_kwargs(mod.one("top_mlp"))
        self.mask_net_layer = MaskNetModule(eg.group_total_dim(self._group), int(n_blocks), mask_block, top_mlp=top,
                                            use_parallel=bool(mod.one("use_parallel", True)))
        self.output_linear = OutputLinear(top["hidden_units"][-1], spec.num_class, bias=False)
        if device is not None:
            for m in (self.mask_net_layer, self.output_linear):
                m.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        features = self.build_input(batch)[self._group]
        return self._output_to_prediction(self.output_linear(self.mask_net_layer(features)))


class ConfigWuKong(RankModel):
    """`wukong {...}` (tzrec/models/wukong.py:36-130): the sparse group as [B, F, D] rows -- the only group, or group `sparse`
    beside an optional group `dense` whose `dense_mlp` output goes first as one more row -- through the WuKong layers, a
    `final` MLP over the flattened last layer, a logits layer with bias.  `wukong { dense_mlp wukong_layers { lcb_feature_num
    fmb_feature_num compressed_feature_num feature_num_mlp } final }` (protos/models/rank_model.proto, module.proto):
    `compressed_feature_num` defaults to 16."""

    _FIELDS = {"wukong": ("dense_mlp", "wukong_layers", "final"),
               "wukong_layers": ("lcb_feature_num", "fmb_feature_num", "compressed_feature_num", "feature_num_mlp")}

    @classmethod
    def _block(cls, parent, where: str, name: str):
        other = sorted(k for k in parent if k not in cls._FIELDS[where])
        if other:
            raise ValueError(f"wukong: {where} has no field {other[0]!r} (fields: {', '.join(cls._FIELDS[where])})")
        if not parent.has(name):
            raise ValueError(f"wukong: {where} needs `{name}`")
        return parent.one(name)

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        names = eg.group_names()
        self._sparse_group = names[0] if len(names) == 1 else "sparse"
        self._dense_group = "dense"
        final = self._block(m, "wukong", "final")
        if not m.many("wukong_layers"):
            raise ValueError("wukong: wukong needs `wukong_layers`")
        self.dense_mlp = None
        if len(names) > 1 and eg.has_group(self._dense_group):
            if any("seq_encoder" in n for n in eg.group_feature_dims(self._dense_group)):
                raise Exception("dense group not have sequence features.")
            self.dense_mlp = mlp_from_msg(eg.group_total_dim(self._dense_group), self._block(m, "wukong", "dense_mlp"))
        sparse_dims = eg.group_feature_dims(self._sparse_group)
        if any("seq_encoder" in n for n in sparse_dims):
            raise Exception("sparse group not have sequence features.")
        dims = set(sparse_dims.values())
        if len(dims) > 1:
            raise Exception(f"sparse group feature dims must be the same, but we find {dims}")
        self._dim = dims.pop()
        self._num_sparse = len(sparse_dims)
        if self.dense_mlp and self._dim != self.dense_mlp.output_dim():
            raise Exception("dense mlp last hidden_unit must be the same sparse feature dim")
        from .wukong import WuKongLayer

        self._wukong_layers = nn.ModuleList()
        feature_num = self._num_sparse + (1 if self.dense_mlp else 0)
        for layer in m.many("wukong_layers"):
            layer = WuKongLayer(self._dim, feature_num, int(self._block(layer, "wukong_layers", "lcb_feature_num")),
                                int(self._block(layer, "wukong_layers", "fmb_feature_num")), int(layer.one("compressed_feature_num", 16)),
                                mlp_kwargs(self._block(layer, "wukong_layers", "feature_num_mlp")))
            self._wukong_layers.append(layer)
            feature_num = layer.output_feature_num()
        self.final_mlp = mlp_from_msg(feature_num * self._dim, final)
        self.output_mlp = OutputLinear(self.final_mlp.output_dim(), spec.num_class)
        if device is not None:
            for mod in (self.dense_mlp, self._wukong_layers, self.final_mlp, self.output_mlp):
                if mod is not None:
                    mod.to(device)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        g = self.build_input(batch)
        feat = g[self._sparse_group].reshape(-1, self._num_sparse, self._dim)
        if self.dense_mlp:
            feat = torch.cat([self.dense_mlp(g[self._dense_group]).unsqueeze(1), feat], dim=1)
        for layer in self._wukong_layers:
            feat = layer(feat)
        return self._output_to_prediction(self.output_mlp(self.final_mlp(feat.reshape(feat.size(0), -1))))


_MODELS = {"dlrm": ConfigDLRM, "deepfm": ConfigDeepFM, "multi_tower_din": ConfigMultiTowerDIN, "mmoe": ConfigMMoE, "ple": ConfigPLE,
           "pepnet": ConfigPEPNet, "dbmtl": ConfigDBMTL,
           "dcn_v1": ConfigDCNV1, "dcn_v2": ConfigDCNV2, "xdeepfm": ConfigXDeepFM, "mask_net": ConfigMaskNet, "wukong": ConfigWuKong}


from .match import ConfigDAT, ConfigDSSM, ConfigMIND  # noqa: E402  (the match models; match.py reads this module's helpers when a tower is built)

_MODELS["dssm"] = ConfigDSSM
_MODELS["mind"] = ConfigMIND
_MODELS["dat"] = ConfigDAT

from . import rocket  # noqa: E402,F401  (rocket.py builds on RankModel and puts _MODELS["rocket_launching"] there itself: either may be imported first)


def build_rank_model(spec: PipelineSpec, device=None, sparse_optimizer=None, process_group=None,
                     plan: Optional[Dict[str, dict]] = None, use_planner: bool = False, exchange: str = "exact") -> RankModel:
    """Class chosen by the model_config oneof name, as tzrec/main.py:151-153 does.  With
    `process_group` the embedding tables are sharded over its ranks (`plan`: planner.plan_tables output
    or None: the planner under the config's `embedding_constraints` / `global_embedding_constraints` when it has
    any or when `use_planner` is set, else the size heuristic) and the dense parameters are kept identical across
    ranks."""
    if spec.model_name not in _MODELS:
        raise NotImplementedError(f"model {spec.model_name!r} is outside SURVEY.md section 8")
    RankModel._build_pg, RankModel._build_plan, RankModel._build_use_planner = process_group, plan, use_planner
    RankModel._build_exchange = exchange  # "capacity": fixed-slice ids exchange for the sharded pooled tables (sharding.py)
    try:
        model = _MODELS[spec.model_name](spec, device, sparse_optimizer)
    finally:
        RankModel._build_pg, RankModel._build_plan, RankModel._build_use_planner = None, None, False
        RankModel._build_exchange = "exact"
    model.sync_dense_parameters()
    return model
