"""The fused sparse optimizer kinds, each described ONCE for the Python side: what embedding.py allocates and passes, what
planner.py and criteo.algorithmic_bytes price.  (The C++ side's table is `bwd_family` of csrc/pooled_bwd_apply.h; the
formulas are in include/tzrec_hip.h.)  No torch import: planner.py reads this and imports numpy alone."""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple


class Kind(NamedTuple):
    code: Optional[int]                  # TZR_OPT_* of include/tzrec_hip.h
    state_width: Callable[[int], int]    # fp32 state floats of a row of D columns
    bwd_row_bytes: Callable[[int], int]  # compulsory HBM bytes of the backward per touched row: weights and state, read and written
    # a [rows, state_width] tensor of its own whatever the row layout; False: no state, or (the Adagrad kinds) placed by the
    # collection's row layout, interleaved with the weights or not (EmbeddingBagCollection._allocate)
    separate_state: bool = True
    state_pad: int = 0                   # floats at the end of the state row that no kernel touches; the row stride is then a multiple of 4
    ticks: bool = False                  # reads the device step state {step, 1 - b1^step, 1 - b2^step}, advanced once per step
    configured_eps: bool = False         # eps comes from the config and divides by itself alone on a zero-gradient row: it must be positive
    slots: Tuple[str, str] = ("beta1", "beta2")  # the SparseOptimizerConfig fields that travel as TzrSparseOptim.beta1 / .beta2
    stride_checked: bool = True          # False for Adam alone, as it always was: check_state_stride does not look at it
    column_priced: bool = True           # False for Adam alone, as it always was: the planner's column-wise option prices its rows without state


KINDS = {
    "sgd": Kind(0, lambda D: 0, lambda D: 8 * D, separate_state=False),
    "adagrad": Kind(1, lambda D: D, lambda D: 16 * D, separate_state=False),
    "rowwise_adagrad": Kind(2, lambda D: 1, lambda D: 8 * D + 8, separate_state=False),
    # [exp_avg | exp_avg_sq].  bwd_row_bytes: priced like SGD, without its state
    "adam": Kind(4, lambda D: 2 * D, lambda D: 8 * D, ticks=True, stride_checked=False, column_priced=False),
    # [exp_avg | exp_avg_sq | pad(3)]: float4 aligned
    "partial_rowwise_adam": Kind(5, lambda D: D + 4, lambda D: 16 * D + 8, state_pad=3, ticks=True),
    "lamb": Kind(6, lambda D: 2 * D, lambda D: 24 * D, ticks=True),  # [exp_avg | exp_avg_sq]
    "partial_rowwise_lamb": Kind(7, lambda D: D + 4, lambda D: 16 * D + 8, state_pad=3, ticks=True),
    "lars_sgd": Kind(8, lambda D: D, lambda D: 16 * D, slots=("momentum", "eta")),  # [momentum]
    # [square_avg | acc_delta]; rho travels in the beta1 slot, beta2 is not read
    "adadelta": Kind(9, lambda D: 2 * D, lambda D: 24 * D, configured_eps=True, slots=("rho", "beta2")),
    "rmsprop": Kind(10, lambda D: D, lambda D: 16 * D, configured_eps=True, slots=("alpha", "beta2")),  # [square_avg]
}
_UNKNOWN = KINDS["sgd"]._replace(code=None)


def of(name: Optional[str]) -> Kind:
    """the record of a kind name; None (no optimizer) or a name nobody knows is laid out and priced like SGD: no state"""
    return KINDS.get(name, _UNKNOWN)
