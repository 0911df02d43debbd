"""The losses a pipeline config names, each as one fused call of csrc/loss_ops.hip (loss + gradient, sample weights inside).

The reference picks a torch module per `losses { ... }` entry (tzrec/models/rank_model.py:181-262) and combines it with the
sample weights in eager torch (rank_model.py:264-287, multi_task_rank.py:97-142): 10-20 elementwise launches per loss, and for
`jrc_loss` several [B, B] tensors (tzrec/loss/jrc_loss.py).  Here:

    binary_cross_entropy (label_smoothing), binary_focal_loss, l2_loss   tzr_loss_pointwise
    softmax_cross_entropy (label_smoothing)                              tzr_softmax_ce
    jrc_loss                                                             tzr_jrc_loss, O(B) memory, after one torch.sort of the session ids

Every call returns the scalar `task_weight * sum(w_i l_i) / sum(w_i)` (0 when the weights sum to 0) with
w_i = sample_weight_i * (indicator_label_i > 0 ? in_task_space_weight : out_task_space_weight) -- the reference's
`mean(l * w / mean(w)) * weight` -- and keeps d(loss)/d(logits) as the unscaled gradient plus a device scalar `scale`, so the
backward is one multiply and nothing syncs with the host.

`jrc_loss` on a batch with no positive (or no negative) row is NaN in the reference's mean form (the mean of an empty tensor
times 0); here it is the finite sum of the rows that exist.

    losses = build_losses(spec)                  # one per LossSpec, in config order
    out = {l.name: l(predictions, batch) for l in losses}
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _lib
from .config import LossSpec, PipelineSpec, TowerSpec

LOSS_BCE, LOSS_FOCAL, LOSS_L2 = 0, 1, 2  # TZR_LOSS_* of include/tzrec_hip.h


class RowWeights:
    """The weight inputs every entry point takes: `weight` float [B] or None, `space_label` (the task-space indicator label)
    or None with its two weights, and the scalar `task_weight`."""

    def __init__(self, weight: Optional[torch.Tensor] = None, space_label: Optional[torch.Tensor] = None, in_w: float = 1.0,
                 out_w: float = 1.0, task_weight: float = 1.0) -> None:
        self.weight = None if weight is None else weight.detach().reshape(-1).contiguous().float()
        self.space_label = None if space_label is None else _label(space_label.detach().reshape(-1))
        self.in_w, self.out_w, self.task_weight = float(in_w), float(out_w), float(task_weight)

    def args(self):
        s = self.space_label
        return (_lib.ptr(self.weight), _lib.ptr(s), s.element_size() if s is not None else 0,
                (1 if s.is_floating_point() else 0) if s is not None else 0, self.in_w, self.out_w, self.task_weight)


_NO_WEIGHTS = RowWeights()


def _label(y: torch.Tensor, integer: bool = False) -> torch.Tensor:
    y = y.contiguous()
    if integer:
        return y if y.dtype in (torch.int32, torch.int64) else y.to(torch.int64)
    return y if y.dtype in (torch.float32, torch.int32, torch.int64) else y.float()


def _outputs(x: torch.Tensor):
    return (torch.empty((), dtype=torch.float32, device=x.device), torch.empty_like(x),
            torch.empty((), dtype=torch.float32, device=x.device))


class _ScaledGradFn(torch.autograd.Function):
    """forward: the entry point's (loss, grad, scale); backward: `grad * (grad_out * scale)`, as _BceLogitsFn's one multiply"""

    @staticmethod
    def forward(ctx, logits, call):
        x = logits.detach().float()
        loss, grad, scale = call(x)
        ctx.save_for_backward(grad, scale)
        ctx.shape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        grad, scale = ctx.saved_tensors
        return (grad * (grad_out * scale)).view(ctx.shape), None


def pointwise_loss(kind: int, logits: torch.Tensor, labels: torch.Tensor, p0: float = 0.0, p1: float = 0.0,
                   weights: RowWeights = _NO_WEIGHTS) -> torch.Tensor:
    """`tzr_loss_pointwise` over [B] logits: kind LOSS_BCE (p0 = label_smoothing), LOSS_FOCAL (p0 = gamma, p1 = alpha), LOSS_L2."""
    y = _label(labels.detach().reshape(-1))

    def call(x):
        x = x.reshape(-1).contiguous()
        if y.numel() != x.numel():
            raise ValueError(f"loss: {x.numel()} logits for {y.numel()} labels")
        loss, grad, scale = _outputs(x)
        L = _lib.lib()
        ws = _lib.workspace(L.tzr_loss_pointwise_workspace(x.numel()), x.device)
        p = _lib.ptr
        _lib.check(L.tzr_loss_pointwise(kind, float(p0), float(p1), p(x), p(y), y.element_size(), 1 if y.is_floating_point() else 0,
                                        *weights.args(), x.numel(), p(loss), p(grad), p(scale), p(ws), ws.numel(),
                                        _lib.stream_ptr(x.device)), "tzr_loss_pointwise")
        return loss, grad, scale

    return _ScaledGradFn.apply(logits, call)


def softmax_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, label_smoothing: float = 0.0, weights: RowWeights = _NO_WEIGHTS,
                          bad_labels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`tzr_softmax_ce` over [B, C] logits (any row stride).  `bad_labels`: an int64 device scalar that counts the labels
    outside [0, C) -- such a row adds nothing to the loss and gets a zero gradient; nothing here reads the counter."""
    y = _label(labels.detach().reshape(-1), integer=True)

    def call(x):
        if x.dim() != 2 or x.shape[0] != y.numel():
            raise ValueError(f"softmax_cross_entropy: logits {tuple(x.shape)} for {y.numel()} labels")
        if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
            x = x.contiguous()
        B, C = x.shape
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        grad = torch.empty((B, C), dtype=torch.float32, device=x.device)
        scale = torch.empty((), dtype=torch.float32, device=x.device)
        L = _lib.lib()
        ws = _lib.workspace(L.tzr_softmax_ce_workspace(B, C), x.device)
        p = _lib.ptr
        _lib.check(L.tzr_softmax_ce(p(x), x.stride(0), C, p(y), y.element_size(), 0, float(label_smoothing), *weights.args(), B,
                                    p(loss), p(grad), p(scale), p(bad_labels), p(ws), ws.numel(), _lib.stream_ptr(x.device)),
                   "tzr_softmax_ce")
        return loss, grad, scale

    return _ScaledGradFn.apply(logits, call)


def jrc_loss(logits: torch.Tensor, labels: torch.Tensor, session_ids: torch.Tensor, alpha: float = 0.5,
             weights: RowWeights = _NO_WEIGHTS) -> torch.Tensor:
    """`tzr_jrc_loss` over [B, 2] logits; a row is positive when its label is 1.  The stable sort of the session ids is torch's
    (plumbing, as GroupedAUC.reduce_rows'); the sessions themselves are found on the device."""
    y = _label(labels.detach().reshape(-1))
    sid = session_ids.detach().reshape(-1).to(torch.int64).contiguous()

    def call(x):
        if x.dim() != 2 or x.shape[1] != 2 or x.shape[0] != y.numel() or sid.numel() != y.numel():
            raise ValueError(f"jrc_loss: logits {tuple(x.shape)}, {y.numel()} labels, {sid.numel()} session ids")
        x = x.contiguous()
        order = torch.sort(sid, stable=True).indices
        loss, grad, scale = _outputs(x)
        L = _lib.lib()
        B = x.shape[0]
        ws = _lib.workspace(L.tzr_jrc_loss_workspace(B), x.device)
        p = _lib.ptr
        _lib.check(L.tzr_jrc_loss(p(x), p(y), y.element_size(), 1 if y.is_floating_point() else 0, p(sid), p(order), float(alpha),
                                  *weights.args(), B, p(loss), p(grad), p(scale), p(ws), ws.numel(), _lib.stream_ptr(x.device)),
                   "tzr_jrc_loss")
        return loss, grad, scale

    return _ScaledGradFn.apply(logits, call)


def session_ids(batch, name: str) -> torch.Tensor:
    """The first id of each sample of sparse feature `name`, 0 for an empty bag (`to_padded_dense(1)[:, 0]`,
    rank_model.py:247-249): the access metrics.Evaluator makes for a `grouping_key`."""
    from .embedding_group import BASE_DATA_GROUP
    from .metrics import first_id_per_sample

    return first_id_per_sample(batch.sparse_features[BASE_DATA_GROUP], name)


class Loss:
    """One configured loss: `loss(predictions, batch) -> scalar`, keyed `name` = kind + `_<tower>`."""

    def __init__(self, ls: LossSpec, label: str, sample_weight_name: Optional[str], tower: Optional[TowerSpec]) -> None:
        self.spec, self.name, self.suffix, self.label = ls, ls.name, ls.suffix, label
        self.sample_weight_name = sample_weight_name
        self.tower = tower
        self.task_weight = tower.weight if tower is not None else 1.0
        self.space_label = tower.task_space_indicator_label if tower is not None else None
        self.bad_labels: Optional[torch.Tensor] = None  # softmax_cross_entropy: labels outside [0, C) seen so far (device int64)

    @property
    def plain_bce(self) -> bool:
        """mean BCE with nothing else: the case that stays on tzr_bce_logits / torch, launch for launch"""
        return (self.spec.kind == "binary_cross_entropy" and not float(self.spec.fields.get("label_smoothing", 0.0)) > 0
                and not self.sample_weight_name and not self.space_label and self.task_weight == 1.0)

    def weights(self, batch) -> RowWeights:
        if not self.sample_weight_name and not self.space_label and self.task_weight == 1.0:
            return _NO_WEIGHTS
        t = self.tower
        return RowWeights(batch.sample_weights[self.sample_weight_name] if self.sample_weight_name else None,
                          batch.labels[self.space_label] if self.space_label else None,
                          t.in_task_space_weight if t is not None else 1.0, t.out_task_space_weight if t is not None else 1.0,
                          self.task_weight)

    def __call__(self, predictions: Dict[str, torch.Tensor], batch) -> torch.Tensor:
        kind, f, s = self.spec.kind, self.spec.fields, self.suffix
        label, w = batch.labels[self.label], self.weights(batch)
        if kind == "binary_cross_entropy":
            return pointwise_loss(LOSS_BCE, predictions["logits" + s], label, max(float(f["label_smoothing"]), 0.0), 0.0, w)
        if kind == "binary_focal_loss":
            return pointwise_loss(LOSS_FOCAL, predictions["logits" + s], label, float(f["gamma"]), float(f["alpha"]), w)
        if kind == "l2_loss":
            return pointwise_loss(LOSS_L2, predictions["y" + s], label, 0.0, 0.0, w)
        if kind == "softmax_cross_entropy":
            x = predictions["logits" + s]
            if self.bad_labels is None or self.bad_labels.device != x.device:
                self.bad_labels = torch.zeros((), dtype=torch.int64, device=x.device)
            return softmax_cross_entropy(x, label, float(f["label_smoothing"]), w, self.bad_labels)
        if kind == "jrc_loss":
            return jrc_loss(predictions["logits" + s], label, session_ids(batch, str(f["session_name"])), float(f["alpha"]), w)
        raise NotImplementedError(f"loss {kind!r}")


def build_losses(spec: PipelineSpec) -> List[Loss]:
    """One `Loss` per `spec.losses` entry, in config order.  A model-level loss reads the first label field and the first of
    `sample_weight_fields` (rank_model.py:78); a tower's its `label_name`, `sample_weight_name`, indicator label and `weight`."""
    out = []
    for ls in spec.losses:
        if ls.tower is None:
            out.append(Loss(ls, spec.label_fields[0] if spec.label_fields else "label",
                            spec.sample_weight_fields[0] if spec.sample_weight_fields else None, None))
        else:
            t = spec.tower(ls.tower)
            out.append(Loss(ls, t.label_name, t.sample_weight_name, t))
    return out


def output_to_prediction(y: torch.Tensor, losses: List[LossSpec], num_class: int, suffix: str = "") -> Dict[str, torch.Tensor]:
    """RankModel._output_to_prediction_impl (rank_model.py:133-167) for every loss of one output: `logits` / `probs` for the binary
    kinds, `logits` / `probs` [B, C] (+ `probs1` when C == 2) for softmax_cross_entropy and jrc_loss, `y` for l2_loss."""
    out: Dict[str, torch.Tensor] = {}
    for ls in losses:
        if ls.kind in ("binary_cross_entropy", "binary_focal_loss"):
            logits = torch.squeeze(y, dim=1)
            out["logits" + suffix], out["probs" + suffix] = logits, torch.sigmoid(logits)
        elif ls.kind in ("softmax_cross_entropy", "jrc_loss"):
            probs = torch.softmax(y, dim=1)
            out["logits" + suffix], out["probs" + suffix] = y, probs
            if num_class == 2:
                out["probs1" + suffix] = probs[:, 1]
        elif ls.kind == "l2_loss":
            out["y" + suffix] = torch.squeeze(y, dim=1)
        else:
            raise NotImplementedError(f"loss {ls.kind!r}")
    return out
