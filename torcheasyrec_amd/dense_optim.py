"""The dense optimizer a tzrec config names, in one fused launch.

The reference turns `train_config.dense_optimizer` into the matching torch.optim class with every field of the block
(tzrec/optim/optimizer_builder.py:100-136) and its `part_optimizers` into further optimizers, each with its own learning-rate
schedule, for the parameters whose names match a regex (:139-260, tzrec/main.py:814-885).  Here the main block and every
part that matched something are the GROUPS of one `FusedDenseOptimizer`, whose step is one launch of tzr_dense_optim_fused
per 32 tensors whatever the mix of kinds; it takes gradients as they lie (`fuse_finish`) and is capturable into a hipGraph,
like `dense.FusedDenseAdam`, whose deferral machinery it shares.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Iterable, List, Optional, Tuple

import torch

from . import _lib, dense, lr_scheduler
from .dense_opt_kinds import DENSE_KINDS, group_options

_NOT_HYPER = ("params", "kind", "part", "initial_lr")


def _n_states(group: dict) -> int:
    k = DENSE_KINDS[group["kind"]]
    return 0 if group["kind"] == "sgd" and group["momentum"] == 0 else len(k.states)


class FusedDenseOptimizer:
    """torch.optim.SGD / Adagrad / Adam / AdamW / Adadelta / RMSprop (single-tensor arithmetic, fp32) over groups of dense
    parameters, each group of its own kind: ONE launch per step (tzr_dense_optim_fused).

    `groups`: dicts with `params`, `kind` (a key of dense_opt_kinds.DENSE_KINDS) and any of the kind's options under
    torch.optim's names (`lr`, `momentum`, `betas`, `weight_decay`, ...); what is left out takes the config proto's default
    (SGD's momentum: 0.9).  At most 8 groups.  `param_groups[i]["lr"]` may be changed between steps: every group's rate is
    mirrored into a device scalar of its own, so a captured hipGraph sees the new value after `sync_lr()`.
    `fuse_finish`: as `dense.FusedDenseAdam`'s."""

    def __init__(self, groups: Iterable[dict], fuse_finish: bool = False) -> None:
        self.param_groups: List[dict] = []
        for g in groups:
            g = dict(g)
            kind = g.get("kind")
            if kind not in DENSE_KINDS:
                raise ValueError(f"Unknown optimizer: {kind}")
            given = {k: v for k, v in g.items() if k not in _NOT_HYPER}
            if "betas" in given:
                given["beta1"], given["beta2"] = given.pop("betas")
            opts = group_options(kind, given)
            self.param_groups.append({"kind": kind, **opts, "params": [p for p in g["params"]],
                                      **{k: g[k] for k in ("part", "initial_lr") if k in g}})
        if len(self.param_groups) > _lib.DENSE_OPT_MAX_GROUPS:
            raise ValueError(f"FusedDenseOptimizer takes at most {_lib.DENSE_OPT_MAX_GROUPS} groups, got {len(self.param_groups)}")
        self.params: List[torch.nn.Parameter] = [p for g in self.param_groups for p in g["params"]]
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError("some parameters appear in more than one parameter group")
        dev = dense._register_fused(self, fuse_finish)
        self.device = dev
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        # per tensor: the kind's state tensors, named as torch.optim names them
        self.state: List[dict] = []
        for gi, p in zip(self._group_of, self.params):
            g = self.param_groups[gi]
            names = DENSE_KINDS[g["kind"]].states[:_n_states(g)]
            fill = g.get("initial_accumulator_value", 0.0)
            self.state.append({n: torch.full_like(p, fill) if n == "sum" else torch.zeros_like(p) for n in names})
        # per tensor: [0] step count, [1 ..] arrival counters of tzr_dense_optim_fused (TZR_ADAM_FUSED_STATE floats, zero between launches)
        self._state = torch.zeros(len(self.params), 40, dtype=torch.float32, device=dev)
        self._lr_dev = torch.tensor([float(g["lr"]) for g in self.param_groups], dtype=torch.float32, device=dev)
        self._lr_host = [float(g["lr"]) for g in self.param_groups]

    def zero_grad(self, set_to_none: bool = True) -> None:
        dense._zero_grad(self.params, set_to_none)

    def sync_lr(self) -> None:
        """Mirror every ``param_groups[i]["lr"]`` into the device scalar the kernel reads for that group.  `step` does it itself
        outside a graph capture; a captured step must not (the fill would be replayed): call this before every replay."""
        for i, g in enumerate(self.param_groups):
            if g["lr"] != self._lr_host[i]:
                self._lr_dev[i:i + 1].fill_(g["lr"])
                self._lr_host[i] = g["lr"]

    def _group_table(self):
        tab = (_lib.TzrDenseOptGroup * len(self.param_groups))()
        for i, g in enumerate(self.param_groups):
            k = DENSE_KINDS[g["kind"]]
            hp = list(g["betas"]) if "betas" in g else [g[n] for n in k.hp]
            hp += [0.0] * (2 - len(hp))
            tab[i].kind, tab[i].flags = k.code, _lib.DENSE_OPT_NESTEROV if g.get("nesterov") else 0
            tab[i].d_lr = self._lr_dev.data_ptr() + 4 * i
            tab[i].lr, tab[i].weight_decay, tab[i].eps = g["lr"], g["weight_decay"], g.get("eps", 0.0)
            tab[i].hp0, tab[i].hp1 = hp[0], hp[1]
        return tab

    def step(self, grads: Optional[List[torch.Tensor]] = None) -> None:
        dense._check_lr_synced(self, any(g["lr"] != h for g, h in zip(self.param_groups, self._lr_host)))
        rows = []
        for i, gr in dense._step_grads(self.params, grads):
            g = self.param_groups[self._group_of[i]]
            if _n_states(g) != len(self.state[i]):
                raise RuntimeError("FusedDenseOptimizer: a group's momentum was switched on or off after construction")
            st = list(self.state[i].values()) + [None, None]
            rows.append(dense._Row(self.params[i].data, gr, st[0], st[1], self._state[i], group=self._group_of[i]))
        if not rows:
            return
        _lib.check_device(self._lr_dev)
        gtab = self._group_table()
        dense._launch_fused(
            rows, lambda part: dense._adam_tables(part, _lib.TzrDenseOptTensor),
            lambda tab, src, wg: _lib.check(_lib.lib().tzr_dense_optim_fused(
                tab, src, len(tab), gtab, len(gtab), C.byref(wg) if wg is not None else None, _lib.stream_ptr(self.device)),
                "tzr_dense_optim_fused"))
        dense._after_fused_step(self)

    def state_dict(self) -> dict:
        """torch.optim's layout: state[i] = {"step", <the kind's state names>}, param_groups with parameter indices"""
        groups, at = [], 0
        for g in self.param_groups:
            groups.append({**{k: v for k, v in g.items() if k != "params"}, "params": list(range(at, at + len(g["params"])))})
            at += len(g["params"])
        return {"state": {i: {"step": self._state[i, 0].clone(), **st} for i, st in enumerate(self.state)}, "param_groups": groups}

    def load_state_dict(self, sd: dict) -> None:
        if len(sd["param_groups"]) != len(self.param_groups) or any(
                a.get("kind", b["kind"]) != b["kind"] or len(a.get("params", b["params"])) != len(b["params"])
                for a, b in zip(sd["param_groups"], self.param_groups)):
            raise ValueError("loaded state dict has other parameter groups than this optimizer")
        self._state[:, 1:].zero_()  # (tzr_dense_optim_fused's arrival counters: zero between launches)
        for i, st in sd["state"].items():
            for n, t in self.state[int(i)].items():
                t.copy_(st[n])
            # (a torch.optim.SGD state has no step: a momentum_buffer in it means the first step is behind)
            self._state[int(i), 0] = float(st["step"]) if "step" in st else float(bool(self.state[int(i)]))
        for a, b in zip(sd["param_groups"], self.param_groups):
            b.update({k: (tuple(v) if k == "betas" else v) for k, v in a.items() if k != "params"})


def group_named_parameters(named_parameters, patterns: List[str]) -> Tuple[list, List[list]]:
    """group_param_by_regex_pattern (tzrec/optim/optimizer_builder.py:219-237): `re.fullmatch` on the parameter's name, the
    first matching pattern wins -> ([(name, param)] that no pattern matched, one such list per pattern)"""
    named = named_parameters.items() if isinstance(named_parameters, dict) else named_parameters
    rest, parts = [], [[] for _ in patterns]
    for name, p in named:
        for i, pat in enumerate(patterns):
            if re.fullmatch(re.compile(pat), name):
                parts[i].append((name, p))
                break
        else:
            rest.append((name, p))
    return rest, parts


def named_dense_parameters(model) -> list:
    """[(name, parameter)] of `model.dense_parameters()` under the names `model.named_parameters()` gives them: what the
    `regex_pattern` of a part optimizer is matched against"""
    dense_ids = {id(p) for p in model.dense_parameters()}
    return [(n, p) for n, p in model.named_parameters() if id(p) in dense_ids]


def build_dense_optimizer(named_parameters, cfg, fuse_finish: bool = False) -> FusedDenseOptimizer:
    """`cfg`: config.DenseOptimizerConfig (spec.dense_optimizer).  Group 0 steps the parameters no `part_optimizers` pattern
    matched with the main block's kind and fields; every part that matched something follows as a group of its own (parts that
    match nothing are dropped, build_part_optimizers :240-260).  A group's "part" entry is its index in cfg.parts, None for
    the main block: `create_dense_schedulers` reads it."""
    rest, parts = group_named_parameters(named_parameters, [p.regex_pattern for p in cfg.parts])
    groups = []
    if rest:
        groups.append({"kind": cfg.kind, **cfg.fields, "params": [p for _, p in rest], "part": None})
    for i, (part, members) in enumerate(zip(cfg.parts, parts)):
        if members:
            groups.append({"kind": part.kind, **part.fields, "params": [p for _, p in members], "part": i})
    return FusedDenseOptimizer(groups, fuse_finish=fuse_finish)


class GroupView:
    """one group of an optimizer as the `optimizer` of a schedule: lr_scheduler.BaseLR writes `param_groups[0]["lr"]`, which IS
    the optimizer's own group dict"""

    def __init__(self, optimizer, index: int) -> None:
        self.optimizer, self.index = optimizer, index
        self.param_groups = [optimizer.param_groups[index]]


def create_dense_schedulers(optimizer, cfg) -> list:
    """One schedule per group of `build_dense_optimizer(..., cfg)`'s optimizer: a part's own `learning_rate` oneof if it has
    one, else the main block's (create_part_optim_schedulers, tzrec/optim/optimizer_builder.py:179-216); a block without the
    oneof gives ConstantLR.  Each schedule drives its group alone."""
    out = []
    for i, g in enumerate(optimizer.param_groups):
        part = g.get("part")
        block = cfg.learning_rate
        if part is not None and lr_scheduler.has_learning_rate(cfg.parts[part].learning_rate):
            block = cfg.parts[part].learning_rate
        out.append(lr_scheduler.create_scheduler(GroupView(optimizer, i), block))
    return out
