"""Rocket Launching (tzrec/models/rocket_launching.py): a wide "booster" net and a small "light" net trained together over one
feature group and an optional shared MLP, the light net pulled towards the booster by a hint loss on the logits and, with
`feature_based_distillation`, one similarity loss per pair of equally wide hidden layers.

`distill_losses` evaluates every distillation term of a step in one autograd Function over tzr_distill_loss_fwd / _bwd
(csrc/distill_loss.hip): one launch and a finishing one forward, one backward, against some ten launches forward and twenty
backward per layer pair in the literal form.  `FUSED_DISTILL_LOSS = False`, operands outside `distill_losses_ok`, or a double
backward run `distill_losses_literal`, the reference's `feature_based_sim` and `_distillation_loss` word for word.
`ConfigRocketLaunching` is the model `build_rank_model` builds from a `rocket_launching { ... }` block.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .config import PipelineSpec
from .dlrm import MLP
from .embedding_group import Batch
from .losses import Loss, output_to_prediction
from .match import _div_no_nan, _literal_grads  # (the reference's div_no_nan and the double-backward path, shared with the match losses)
from .rank_model import RankModel, mlp_kwargs

FUSED_DISTILL_LOSS = True  # profiles/distill_loss: the fused form against the literal one, without and with sample weights


def feature_based_sim(light_feature: torch.Tensor, booster_feature: torch.Tensor, loss_weight: Optional[torch.Tensor], cosine: bool):
    """tzrec/models/rocket_launching.py:125-155, word for word"""
    booster_feature_no_gradient = booster_feature.detach()
    if cosine:
        booster_feature_no_gradient_norm = F.normalize(booster_feature_no_gradient, p=2, dim=1)
        light_feature_norm = F.normalize(light_feature, p=2, dim=1)
        multi_middle_layer = torch.mul(booster_feature_no_gradient_norm, light_feature_norm)
        if loss_weight is not None:
            sim_middle_layer = -0.1 * torch.mean(torch.sum(multi_middle_layer, dim=1) * loss_weight)
        else:
            sim_middle_layer = -0.1 * torch.mean(torch.sum(multi_middle_layer, dim=1))
        return sim_middle_layer
    else:
        distance_square = torch.square(booster_feature_no_gradient - light_feature)
        if loss_weight is not None:
            distance_square = torch.sum(distance_square, dim=1) * loss_weight
        return torch.sqrt(torch.sum(distance_square))


def distill_losses_literal(light_feats: Sequence[torch.Tensor], booster_feats: Sequence[torch.Tensor], logits_light: torch.Tensor,
                           logits_booster: torch.Tensor, cosine: bool, weights: Optional[torch.Tensor] = None):
    """the reference's `loss` weight (rocket_launching.py:211-215), `feature_based_sim` per pair and `_distillation_loss`'s hint
    (rocket_launching.py:194-203) -> (sims, hint)"""
    loss_weight = None if weights is None else _div_no_nan(weights, torch.mean(weights))
    sims = tuple(feature_based_sim(l, b, loss_weight, cosine) for l, b in zip(light_feats, booster_feats))
    batch_hint_loss = F.mse_loss(logits_light, logits_booster.detach(), reduction="none" if loss_weight is not None else "mean")
    hint = torch.mean(batch_hint_loss * loss_weight) if loss_weight is not None else batch_hint_loss
    return sims, hint


def distill_losses_ok(light_feats: Sequence[torch.Tensor], booster_feats: Sequence[torch.Tensor], logits_light: torch.Tensor,
                      logits_booster: torch.Tensor, weights: Optional[torch.Tensor] = None) -> bool:
    """what tzr_distill_loss_* takes: at most 8 pairs of fp32 [B, W_p] tensors with unit column stride, row strides that are
    multiples of 4 floats and 16-byte aligned rows (column slices of wider buffers are fine), W_p % 4 == 0, 4 <= W_p <= 1024;
    logits fp32 contiguous, [B] (C = 1) or [B, C <= 64], of one shape; B >= 1; weights fp32 [B] contiguous and then C == 1 (the
    reference's [B, C] * [B] does not broadcast); everything on the device of the loaded library"""
    if len(light_feats) != len(booster_feats) or len(light_feats) > _lib.DISTILL_MAX_PAIRS:
        return False
    if logits_light.dim() not in (1, 2) or logits_light.shape != logits_booster.shape:
        return False
    B, dev = logits_light.shape[0], logits_light.device
    Cn = 1 if logits_light.dim() == 1 else logits_light.shape[1]
    if not _lib.takes(dev) or B < 1 or not 1 <= Cn <= _lib.DISTILL_MAX_C:
        return False
    for t in (logits_light, logits_booster):
        if not (t.dtype == torch.float32 and t.is_contiguous() and t.device == dev):
            return False
    for l, b in zip(light_feats, booster_feats):
        if not (l.dim() == 2 and _lib.rows_ok(l) and _lib.rows_ok(b, l.shape[1]) and l.shape[0] == b.shape[0] == B
                and l.device == dev and b.device == dev):
            return False
        if not (l.shape[1] % 4 == 0 and 4 <= l.shape[1] <= _lib.DISTILL_MAX_W):
            return False
    return weights is None or (_lib.packed_ok(weights, (B,), dev) and logits_light.dim() == 1)


class _DistillLossFn(torch.autograd.Function):
    """Inputs: logits_light (gradient), logits_booster, weights or None (constants), `cosine`, P, then P light tensors (gradients)
    and P booster tensors (constants).  Outputs: sim_0 .. sim_{P-1}, hint (scalars).  Saved for the backward: the inputs and 1 +
    8 floats -- nothing per sample, the backward recomputes the norms from the rows it reads anyway.  Capturable: the upstream
    gradients are read from device memory, every buffer is torch's.  Asked for a double backward, the backward differentiates the
    literal form instead."""

    @staticmethod
    def _fill(m, logits_light, logits_booster, weights, cosine, lights, boosters, scale):
        m.B, m.P, m.cosine = logits_light.shape[0], len(lights), int(cosine)
        m.C = 1 if logits_light.dim() == 1 else logits_light.shape[1]
        for p, (l, b) in enumerate(zip(lights, boosters)):
            m.W[p] = l.shape[1]
            m.light[p], m.light_stride[p], m.booster[p], m.booster_stride[p] = _lib.ptr(l), l.stride(0), _lib.ptr(b), b.stride(0)
        m.logits_light, m.logits_booster = _lib.ptr(logits_light), _lib.ptr(logits_booster)
        m.w = _lib.opt_ptr(weights)
        m.scale = _lib.ptr(scale)

    @staticmethod
    def forward(ctx, logits_light, logits_booster, weights, cosine, P, *feats):
        lights, boosters = feats[:P], feats[P:]
        dev = logits_light.device
        loss = torch.empty(P + 1, dtype=torch.float32, device=dev)
        scale = torch.empty(1 + _lib.DISTILL_MAX_PAIRS, dtype=torch.float32, device=dev)
        m = _lib.TzrDistillLoss()
        _DistillLossFn._fill(m, logits_light, logits_booster, weights, cosine, lights, boosters, scale)
        m.loss = _lib.ptr(loss)
        _lib.launch_ws("tzr_distill_loss", m, dev, "tzr_distill_loss_fwd")
        ctx.save_for_backward(logits_light, logits_booster, weights, scale, *feats)
        ctx.cfg = (cosine, P)
        ctx.set_materialize_grads(False)  # (no zero-filled gradient for a term nobody reads: a launch)
        return tuple(loss[i] for i in range(P + 1))

    @staticmethod
    def backward(ctx, *grads):
        logits_light, logits_booster, weights, scale = ctx.saved_tensors[:4]
        cosine, P = ctx.cfg
        feats = ctx.saved_tensors[4:]
        lights, boosters = feats[:P], feats[P:]
        need_ll, need_l = ctx.needs_input_grad[0], ctx.needs_input_grad[5:5 + P]
        none = (None,) * P
        if all(g is None for g in grads):
            return (None,) * 5 + none + none
        if torch.is_grad_enabled():  # (create_graph: a double backward is coming)
            sims, hint = distill_losses_literal(lights, boosters, logits_light, logits_booster, cosine, weights)
            got = _literal_grads(sims + (hint,), grads, (logits_light,) + tuple(lights), (need_ll,) + tuple(need_l), allow_unused=True)
            return (got[0], None, None, None, None) + got[1:] + none
        dev = logits_light.device
        grads = [None if g is None else g.to(torch.float32) for g in grads]
        m = _lib.TzrDistillLoss()
        _DistillLossFn._fill(m, logits_light, logits_booster, weights, cosine, lights, boosters, scale)
        d_lights = []
        for p in range(P):
            want = need_l[p] and grads[p] is not None
            d = torch.empty(lights[p].shape, dtype=torch.float32, device=dev) if want else None
            d_lights.append(d)
            m.grad_sim[p] = _lib.opt_ptr(grads[p])
            m.dlight[p], m.dlight_stride[p] = (_lib.ptr(d), d.stride(0)) if want else (0, 0)
        d_ll = torch.empty_like(logits_light) if need_ll and grads[P] is not None else None
        m.grad_hint, m.dlogits_light = _lib.opt_ptr(grads[P]), _lib.opt_ptr(d_ll)
        _lib.launch("tzr_distill_loss_bwd", m, dev)
        return (d_ll, None, None, None, None) + tuple(d_lights) + none


def distill_losses(light_feats: Sequence[torch.Tensor], booster_feats: Sequence[torch.Tensor], logits_light: torch.Tensor,
                   logits_booster: torch.Tensor, cosine: bool, weights: Optional[torch.Tensor] = None):
    """Rocket Launching's distillation terms -> (sims: tuple of one scalar per pair, hint).  light_feats[p] / booster_feats[p]
    [B, W_p]: a pair of equally wide hidden layers; logits [B] or [B, C]; `weights` [B] sample weights, divided by their mean
    inside (0 where the mean is 0).  `cosine`: sim_p = -0.1 mean(lw <normalize(light), normalize(booster)>), else sqrt(sum(lw
    |booster - light|^2)); hint = mean(lw (logits_light - logits_booster)^2).  The booster operands are treated as detached.  One
    launch and a finishing one forward, one backward, unless FUSED_DISTILL_LOSS is off or `distill_losses_ok` refuses the
    operands: then the literal form runs.  Distance mode with a total of exactly 0: the fused gradient is zero rows, the literal
    one NaN."""
    light_feats = tuple(light_feats)
    booster_feats = tuple(b.detach() for b in booster_feats)
    logits_booster = logits_booster.detach()
    if weights is not None:
        weights = weights.detach()
    if FUSED_DISTILL_LOSS and distill_losses_ok(light_feats, booster_feats, logits_light, logits_booster, weights):
        out = _DistillLossFn.apply(logits_light, logits_booster, weights, bool(cosine), len(light_feats), *light_feats, *booster_feats)
        return tuple(out[:-1]), out[-1]
    return distill_losses_literal(light_feats, booster_feats, logits_light, logits_booster, bool(cosine), weights)


class ConfigRocketLaunching(RankModel):
    """`rocket_launching { share_mlp {} booster_mlp {} light_mlp {} feature_based_distillation feature_distillation_function }`
    (tzrec/models/rocket_launching.py:38-245, protos/models/rank_model.proto: RocketLaunching) over the first feature group.
    `share_mlp` is optional; `booster_linear` / `light_linear` map to `num_class` outputs with bias.  The light net reads
    `share_net.detach()`: the tables and the shared MLP take gradient from the booster alone.  Light layer i is paired with the
    first booster layer j of equal width.

    `forward(batch)` in training mode: `logits` / `probs` (`probs1`, `y`: as `output_to_prediction` gives per loss kind) with the
    suffixes `_light` and `_booster`, and with `feature_based_distillation` the paired hidden layers `light_<i>` / `booster_<j>`.
    Under `eval()` the `_light` entries alone; the booster does not run.  `loss(predictions, batch)`: `<kind>_booster` (training)
    and `<kind>_light` per configured loss, each a fused call of losses.py with the first sample weight field, plus in training
    `hint_l2_loss` and `similarity_<i>_<j>` from `distill_losses`.  `feature_distillation_function`: COSINE (the default) is the
    cosine branch, every other value the distance branch (the reference's `else`).

    Two deliberate differences (NOTES.md).  With `feature_based_distillation: false` no hidden layer is published and the hint
    loss alone is added; the reference's training forward raises there whenever two widths agree (it indexes a tensor by a
    string).  Sample weights with `num_class > 1` are refused when the model is built: the reference multiplies a [B, C] hint by
    [B] weights, which broadcasts only when B == C.  Also refused by name: a missing `booster_mlp` or `light_mlp`."""

    _FIELDS = ("share_mlp", "booster_mlp", "light_mlp", "feature_based_distillation", "feature_distillation_function")

    def __init__(self, spec: PipelineSpec, device=None, sparse_optimizer=None) -> None:
        super().__init__(spec, device, sparse_optimizer)
        eg, m = self.embedding_group, spec.model
        other = sorted(k for k in m if k not in self._FIELDS)
        if other:
            raise ValueError(f"rocket_launching: no field {other[0]!r} (fields: {', '.join(self._FIELDS)})")
        for k in ("booster_mlp", "light_mlp"):
            if not m.has(k):
                raise ValueError(f"rocket_launching: needs `{k}` (required in the proto)")
        self._weight = spec.sample_weight_fields[0] if spec.sample_weight_fields else None
        if self._weight and spec.num_class > 1:
            raise ValueError(f"rocket_launching: sample weights ({self._weight!r}) with num_class {spec.num_class}: the hint loss would "
                             "multiply [B, num_class] by [B] weights, which the reference can only do when the two are equal")
        self._feature_based = bool(m.one("feature_based_distillation", False))
        self._cosine = str(m.one("feature_distillation_function", "COSINE")) == "COSINE"
        self._group = eg.group_names()[0]
        d_in = eg.group_total_dim(self._group)
        self.share_mlp = MLP(d_in, **mlp_kwargs(m.one("share_mlp"))) if m.has("share_mlp") else None
        d = self.share_mlp.output_dim() if self.share_mlp is not None else d_in
        self.booster_mlp = MLP(d, return_hidden_layer_feature=self._feature_based, **mlp_kwargs(m.one("booster_mlp")))
        self.booster_linear = nn.Linear(self.booster_mlp.output_dim(), spec.num_class)
        self.light_mlp = MLP(d, return_hidden_layer_feature=self._feature_based, **mlp_kwargs(m.one("light_mlp")))
        self.light_linear = nn.Linear(self.light_mlp.output_dim(), spec.num_class)
        # rocket_launching.py:77-86: light layer i with the first booster layer j of equal width
        self.mlp_index_dict: Dict[int, int] = {}
        for i, unit_i in enumerate(self.light_mlp.hidden_units):
            for j, unit_j in enumerate(self.booster_mlp.hidden_units):
                if unit_i == unit_j:
                    self.mlp_index_dict[i] = j
                    break
        self._pairs = sorted(self.mlp_index_dict.items()) if self._feature_based else []
        label = spec.label_fields[0] if spec.label_fields else "label"
        self._side_losses = {}
        for suffix in ("_booster", "_light"):
            side = []
            for l in self._model_losses:
                sl = Loss(l.spec, label, self._weight, None)
                sl.suffix, sl.name = suffix, l.spec.kind + suffix
                side.append(sl)
            self._side_losses[suffix] = side
        if device is not None:
            for mod in (self.share_mlp, self.booster_mlp, self.booster_linear, self.light_mlp, self.light_linear):
                if mod is not None:
                    mod.to(device)

    def metric_suffixes(self):
        """which predictions the config's model-level metrics read in evaluation -- what metrics.Evaluator measures, whose
        `evaluate` puts the model into eval mode -- : `_light` alone, the booster does not run (rocket_launching.py:260-277)"""
        return ["_light"]

    def _side(self, mlp: MLP, linear: nn.Linear, x: torch.Tensor, suffix: str):
        net = mlp(x)
        out = linear(net["hidden_layer_end"] if self._feature_based else net)
        return net, output_to_prediction(out, [l.spec for l in self._model_losses], self._spec.num_class, suffix=suffix)

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        net = self.build_input(batch)[self._group]
        share_net = self.share_mlp(net) if self.share_mlp is not None else net
        light_net, predictions = self._side(self.light_mlp, self.light_linear, share_net.detach(), "_light")
        if self.training:
            booster_net, booster = self._side(self.booster_mlp, self.booster_linear, share_net, "_booster")
            predictions.update(booster)
            for i, j in self._pairs:
                predictions[f"light_{i}"] = light_net[f"hidden_layer{i}"]
                predictions[f"booster_{j}"] = booster_net[f"hidden_layer{j}"]
        return predictions

    def loss(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        out = {}
        for k in range(len(self._model_losses)):
            if self.training:
                l = self._side_losses["_booster"][k]
                out[l.name] = l(predictions, batch)
            l = self._side_losses["_light"][k]
            out[l.name] = l(predictions, batch)
        if self.training:
            weights = batch.sample_weights[self._weight].to(torch.float32) if self._weight else None
            sims, hint = distill_losses([predictions[f"light_{i}"] for i, _ in self._pairs],
                                        [predictions[f"booster_{j}"] for _, j in self._pairs],
                                        predictions["logits_light"], predictions["logits_booster"], self._cosine, weights)
            for (i, j), s in zip(self._pairs, sims):
                out[f"similarity_{i}_{j}"] = s
            out["hint_l2_loss"] = hint
        return out


from . import rank_model as _rank_model  # noqa: E402  (registered here, not in rank_model.py: either module may be imported first)

_rank_model._MODELS["rocket_launching"] = ConfigRocketLaunching
