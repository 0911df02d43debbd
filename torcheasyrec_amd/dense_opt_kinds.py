"""The dense optimizer kinds, each described ONCE for the Python side: what config.py reads out of a `dense_optimizer` /
`part_optimizers` block, what dense_optim.FusedDenseOptimizer allocates and passes.  (The kernel's side is the switch of
csrc/dense_optim_fused.hip; the formulas are in include/tzrec_hip.h.)  No torch import, like opt_kinds.py."""
from __future__ import annotations

from typing import Dict, NamedTuple, Tuple


class DenseKind(NamedTuple):
    code: int                  # TZR_DENSE_OPT_* of include/tzrec_hip.h
    states: Tuple[str, ...]    # the fp32 state tensors (state0, state1), named as torch.optim's state_dict names them
    fields: Dict[str, object]  # the config message's fields with the proto's defaults (protos/optimizer.proto:159-208), `fused` aside
    hp: Tuple[str, ...] = ()   # the param-group entries that travel as TzrDenseOptGroup.hp0 / .hp1


_ADAM = {"lr": 0.002, "beta1": 0.9, "beta2": 0.999, "weight_decay": 0.0, "eps": 1e-8, "amsgrad": False}

DENSE_KINDS = {
    # momentum_buffer only when momentum != 0
    "sgd": DenseKind(0, ("momentum_buffer",), {"lr": 0.002, "momentum": 0.9, "weight_decay": 0.0, "dampening": 0.0, "nesterov": False},
                     ("momentum", "dampening")),
    # `sum` starts at initial_accumulator_value; eps is not read by the kernel's hp slots: TzrDenseOptGroup.eps
    "adagrad": DenseKind(1, ("sum",), {"lr": 0.002, "weight_decay": 0.0, "initial_accumulator_value": 0.0, "eps": 1e-10}),
    "adam": DenseKind(2, ("exp_avg", "exp_avg_sq"), dict(_ADAM), ("beta1", "beta2")),
    "adamw": DenseKind(3, ("exp_avg", "exp_avg_sq"), dict(_ADAM), ("beta1", "beta2")),
    "adadelta": DenseKind(4, ("square_avg", "acc_delta"), {"lr": 0.002, "rho": 0.95, "eps": 1e-6, "weight_decay": 0.0}, ("rho",)),
    "rmsprop": DenseKind(5, ("square_avg",), {"lr": 0.002, "alpha": 0.99, "eps": 1e-8, "weight_decay": 0.0}, ("alpha",)),
}
# fields of a config message that select torch's implementation, not the arithmetic: accepted and dropped
IMPLEMENTATION_FIELDS = ("fused",)


def group_options(kind: str, fields: Dict[str, object]) -> Dict[str, object]:
    """config fields (any subset; the rest take the proto's defaults) -> the entries of a `param_groups` group under torch.optim's
    keys: beta1 / beta2 become `betas`, everything else keeps its name.  `amsgrad: true` is refused by name."""
    k = DENSE_KINDS[kind]
    unknown = [f for f in fields if f not in k.fields and f not in IMPLEMENTATION_FIELDS]
    if unknown:
        raise ValueError(f"{kind}_optimizer: unknown field(s) {unknown}")
    o = {f: type(d)(fields.get(f, d)) if not isinstance(d, bool) else _bool(fields.get(f, d)) for f, d in k.fields.items()}
    if o.pop("amsgrad", False):
        raise ValueError(f"{kind}_optimizer: amsgrad: true is not supported by the fused dense optimizer (no kernel keeps max_exp_avg_sq)")
    if "beta1" in o:
        o["betas"] = (o.pop("beta1"), o.pop("beta2"))
    if kind == "sgd" and o["nesterov"] and (o["momentum"] <= 0 or o["dampening"] != 0):
        raise ValueError("sgd_optimizer: nesterov momentum requires a momentum and zero dampening")  # (torch.optim.SGD's own rule)
    return o


def _bool(v) -> bool:
    return v if isinstance(v, bool) else str(v).lower() == "true"
