"""The match (retrieval) models: the fused similarity head, MIND's label-aware attention, DAT's Adaptive-Mimic loss, and DSSM, MIND and
DAT built from their configs.

`match_softmax` is the head of tzrec/models/match_model.py:50-64, 303-336 and dssm.py:81-83, 147-155 -- normalize,
similarity, temperature, softmax cross entropy -- plus the rank of the positive that recall@k needs, in one autograd Function over
tzr_match_softmax_fwd / _bwd (csrc/match_softmax.hip): the [B, 1 + N] (or [B, B]) score matrix is never in memory unless the
caller asks for it.  `FUSED_MATCH_SOFTMAX = False`, or a shape outside `match_softmax_ok`, runs the reference's literal form.
`label_attention` (tzrec/models/mind.py:303-333, tzr_label_attn_fwd / _bwd, csrc/label_attention.hip) is switched the same way by
`FUSED_LABEL_ATTENTION` and `label_attention_ok`; MIND's capsule layer is capsule.py's.  `amm_loss` (tzrec/models/dat.py:212-259,
tzr_amm_loss_fwd / _bwd, csrc/amm_loss.hip) likewise by `FUSED_AMM_LOSS` and `amm_loss_ok`.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .capsule import CapsuleConfig, CapsuleLayer
from .embedding_group import BASE_DATA_GROUP, Batch, EmbeddingGroup

SAMPLED, IN_BATCH = _lib.MATCH_SAMPLED, _lib.MATCH_IN_BATCH
FUSED_MATCH_SOFTMAX = True  # profiles/match_softmax: the fused head against the literal one at both modes' example shapes


def match_softmax_ok(user: torch.Tensor, item: torch.Tensor, mode: int, weights: Optional[torch.Tensor] = None) -> bool:
    """what tzr_match_softmax_* takes: fp32 user [B, D] and item [M, D] with unit column stride, row strides that are multiples of
    4 floats and 16-byte aligned rows (column slices of wider buffers are fine); D % 4 == 0, 4 <= D <= 256; B >= 1; M >= B in
    SAMPLED mode (N = M - B negatives, N = 0 allowed), M == B in IN_BATCH mode; weights fp32 [B] contiguous; everything on the
    device of the loaded library"""
    if user.dim() != 2 or item.dim() != 2:
        return False
    B, D = user.shape
    if not _lib.takes(user) or item.device != user.device:
        return False
    if not (D % 4 == 0 and 4 <= D <= _lib.MATCH_SOFTMAX_MAX_D and B >= 1 and _lib.rows_ok(user, D) and _lib.rows_ok(item, D)):
        return False
    M = item.shape[0]
    if mode == SAMPLED:
        if M < B:
            return False
    elif mode == IN_BATCH:
        if M != B:
            return False
    else:
        return False
    return weights is None or _lib.packed_ok(weights, (B,), user.device)


def match_scores(user: torch.Tensor, item: torch.Tensor, mode: int, cosine: bool, temperature: float) -> torch.Tensor:
    """the reference's literal score matrix (match_model.py:50-64, dssm.py:81-83, 147-155): [B, 1 + N] in SAMPLED mode (column 0
    the positive), [B, B] in IN_BATCH mode"""
    if cosine:
        user, item = F.normalize(user, p=2.0, dim=1), F.normalize(item, p=2.0, dim=1)
    if mode == IN_BATCH:
        sim = torch.mm(user, item.T)
    else:
        B = user.shape[0]
        pos = torch.sum(user * item[:B], dim=-1, keepdim=True)
        neg = torch.matmul(user, item[B:].T)
        sim = torch.cat([pos, neg], dim=-1)
    return sim / temperature


def scores_loss_rank(sim: torch.Tensor, mode: int, weights: Optional[torch.Tensor] = None):
    """(loss, rank) of a materialised score matrix: the reference's CrossEntropyLoss against label 0 (SAMPLED) or arange(B)
    (IN_BATCH), with sample weights mean(l w) / mean(w) (0 where that denominator is 0); rank_i = the number of other columns
    strictly above the label's"""
    B = sim.shape[0]
    label = torch.arange(B, device=sim.device) if mode == IN_BATCH else torch.zeros(B, dtype=torch.long, device=sim.device)
    if weights is None:
        loss = F.cross_entropy(sim, label)
    else:
        rows = F.cross_entropy(sim, label, reduction="none")
        num, den = torch.mean(rows * weights), torch.mean(weights)
        loss = torch.where(den != 0, num / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(num))
    pos = sim.gather(1, label[:, None])
    rank = (sim > pos).sum(dim=1).to(torch.int32)  # (the label's own column is not above itself)
    return loss, rank


def _literal(user, item, mode, cosine, temperature, weights, want_sim):
    sim = match_scores(user, item, mode, cosine, temperature)
    loss, rank = scores_loss_rank(sim, mode, weights)
    return loss, rank.detach(), (sim if want_sim else None)


class _MatchSoftmaxFn(torch.autograd.Function):
    """Inputs: user [B, D], item [M, D], weights [B] or None.  Outputs: loss (scalar), rank [B] int32, sim [B, C] or an empty
    tensor; only the loss carries a gradient.  Saved for the backward: the inputs and O(B + M) floats (lse, pos, the inverse
    norms, the loss's denominator).  Capturable: the upstream gradient is read from device memory, every buffer is torch's."""

    @staticmethod
    def _fill(m, user, item, weights, mode, cosine, temperature, saved):
        lse, rmax, lsum, pos, scale, ru, rv = saved
        m.B, m.M, m.D, m.mode, m.cosine = user.shape[0], item.shape[0], user.shape[1], mode, int(cosine)
        m.inv_temperature = 1.0 / float(temperature)
        m.u, m.u_stride, m.v, m.v_stride = _lib.ptr(user), user.stride(0), _lib.ptr(item), item.stride(0)
        m.w = _lib.opt_ptr(weights)
        m.lse, m.rmax, m.lsum, m.pos, m.scale = _lib.ptr(lse), _lib.ptr(rmax), _lib.ptr(lsum), _lib.ptr(pos), _lib.ptr(scale)
        if cosine:
            m.ru, m.rv = _lib.ptr(ru), _lib.ptr(rv)

    @staticmethod
    def forward(ctx, user, item, weights, mode, cosine, temperature, want_sim):
        B, D = user.shape
        M, dev = item.shape[0], user.device
        f32 = dict(dtype=torch.float32, device=dev)
        loss, scale = torch.empty((), **f32), torch.empty(1, **f32)
        rows = torch.empty(4, B, **f32)
        lse, rmax, lsum, pos = rows.unbind(0)
        rank = torch.empty(B, dtype=torch.int32, device=dev)
        ru, rv = (torch.empty(B, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)) if cosine else (None, None)
        sim = torch.empty(B, (1 + M - B) if mode == SAMPLED else M, **f32) if want_sim else torch.empty(0, **f32)
        m = _lib.TzrMatchSoftmax()
        _MatchSoftmaxFn._fill(m, user, item, weights, mode, cosine, temperature, (lse, rmax, lsum, pos, scale, ru, rv))
        m.loss, m.rank = _lib.ptr(loss), _lib.ptr(rank)
        if want_sim:
            m.sim, m.sim_stride = _lib.ptr(sim), sim.stride(0)
        _lib.launch_ws("tzr_match_softmax", m, dev, "tzr_match_softmax_fwd")
        ctx.save_for_backward(user, item, weights, rows, scale, ru, rv)
        ctx.cfg = (mode, cosine, temperature)
        ctx.mark_non_differentiable(rank, sim)
        return loss, rank, sim

    @staticmethod
    def backward(ctx, gloss, _grank, _gsim):
        user, item, weights, rows, scale, ru, rv = ctx.saved_tensors
        lse, rmax, lsum, pos = rows.unbind(0)
        mode, cosine, temperature = ctx.cfg
        dev = user.device
        g = gloss.to(torch.float32).reshape(1).contiguous()
        du, dv = torch.empty(user.shape, dtype=torch.float32, device=dev), torch.empty(item.shape, dtype=torch.float32, device=dev)
        m = _lib.TzrMatchSoftmax()
        _MatchSoftmaxFn._fill(m, user, item, weights, mode, cosine, temperature, (lse, rmax, lsum, pos, scale, ru, rv))
        m.grad_loss = _lib.ptr(g)
        m.du, m.du_stride, m.dv, m.dv_stride = _lib.ptr(du), du.stride(0), _lib.ptr(dv), dv.stride(0)
        _lib.launch("tzr_match_softmax_bwd", m, dev)
        return du, dv, None, None, None, None, None


def match_softmax(user: torch.Tensor, item: torch.Tensor, mode: int, cosine: bool, temperature: float,
                  weights: Optional[torch.Tensor] = None, want_sim: bool = False):
    """-> (loss, rank, sim or None).  user [B, D]: the user tower's output before any normalisation; item [M, D]: the item
    tower's, M = B + N in SAMPLED mode (row i the positive of user row i, rows B.. the shared negatives), M = B in IN_BATCH mode.
    loss: the reference's softmax cross entropy (with `weights` [B]: mean(l w) / mean(w), 0 where mean(w) is 0); rank [B] int32: the
    number of other columns strictly above the positive's score; sim: the [B, C] scores when `want_sim`.  One launch and a
    finishing one forward, two backward, unless FUSED_MATCH_SOFTMAX is off or `match_softmax_ok` refuses the shape: then the
    literal normalize / sim / cross_entropy form runs."""
    if weights is not None:
        weights = weights.detach()
    if FUSED_MATCH_SOFTMAX and match_softmax_ok(user, item, mode, weights):
        loss, rank, sim = _MatchSoftmaxFn.apply(user, item, weights, mode, bool(cosine), float(temperature), bool(want_sim))
        return loss, rank, (sim if want_sim else None)
    return _literal(user, item, mode, bool(cosine), float(temperature), weights, want_sim)


FUSED_LABEL_ATTENTION = True  # profiles/capsule: with the capsule layer, against the literal forms


def label_attention_literal(interests: torch.Tensor, item: torch.Tensor, mask: torch.Tensor, simi_pow: float) -> torch.Tensor:
    """tzrec/models/mind.py:303-333, word for word"""
    pos_item_emb = item[:interests.size(0)]
    interest_weight = torch.einsum("bkd, bd->bk", interests, pos_item_emb)
    threshold = (mask.to(interests.dtype) * 2 - 1) * float("inf")
    interest_weight = torch.minimum(interest_weight, threshold)
    interest_weight = interest_weight.unsqueeze(-1) * simi_pow
    interest_weight = torch.nn.functional.softmax(interest_weight, dim=1)
    return torch.sum(torch.multiply(interest_weight, interests), dim=1)


def label_attention_ok(interests: torch.Tensor, item: torch.Tensor, mask: torch.Tensor, simi_pow: float) -> bool:
    """what tzr_label_attn_* takes: fp32 interests [B, K, D] whose B K rows have one stride (a multiple of 4 floats, 16-byte
    aligned; a column slice of a [B K, .] buffer is fine), item [M >= B, D] rows likewise, mask [B, K] bool contiguous; D % 4 == 0,
    4 <= D <= 256, 1 <= K <= 8, B >= 1, simi_pow > 0; everything on the device of the loaded library"""
    if interests.dim() != 3 or item.dim() != 2 or mask.dim() != 2:
        return False
    B, K, D = interests.shape
    if not _lib.takes(interests) or item.device != interests.device or mask.device != interests.device:
        return False
    if not (D % 4 == 0 and 4 <= D <= _lib.LABEL_ATTN_MAX_D and 1 <= K <= _lib.LABEL_ATTN_MAX_K and B >= 1 and simi_pow > 0):
        return False
    return bool(_lib.rows3_ok(interests) and item.shape[0] >= B and _lib.rows_ok(item, D) and mask.shape == (B, K) and mask.dtype == torch.bool
                and mask.is_contiguous())


class _LabelAttentionFn(torch.autograd.Function):
    """Inputs: interests [B, K, D], item [M, D], mask [B, K] bool.  Outputs: user_emb [B, D] and the weights w [B, K] (saved for
    the backward, no gradient).  The item gradient is zero behind its first B rows."""

    @staticmethod
    def forward(ctx, interests, item, mask, simi_pow):
        B, K, D = interests.shape
        dev = interests.device
        out = torch.empty(B, D, dtype=torch.float32, device=dev)
        w = torch.empty(B, K, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().tzr_label_attn_fwd(_lib.ptr(interests), interests.stride(1), _lib.ptr(item), item.stride(0), _lib.ptr(mask), B, K, D,
                                                 float(simi_pow), _lib.ptr(out), D, _lib.ptr(w), _lib.stream_ptr(dev)), "tzr_label_attn_fwd")
        ctx.save_for_backward(interests, item, mask, w)
        ctx.simi_pow = float(simi_pow)
        ctx.mark_non_differentiable(w)
        ctx.set_materialize_grads(False)  # (no zero-filled gradient for w: a launch a pass)
        return out, w

    @staticmethod
    def backward(ctx, gout, _gw):
        if gout is None:
            return None, None, None, None
        interests, item, mask, w = ctx.saved_tensors
        B, K, D = interests.shape
        dev = interests.device
        g = _lib.rows16(gout.to(torch.float32))
        di = torch.empty(B, K, D, dtype=torch.float32, device=dev)
        dv = torch.zeros(item.shape, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().tzr_label_attn_bwd(_lib.ptr(g), g.stride(0), _lib.ptr(interests), interests.stride(1), _lib.ptr(item), item.stride(0),
                                                 _lib.ptr(w), _lib.ptr(mask), B, K, D, ctx.simi_pow, _lib.ptr(di), D, _lib.ptr(dv), D,
                                                 _lib.stream_ptr(dev)), "tzr_label_attn_bwd")
        return di, dv, None, None


def label_attention(interests: torch.Tensor, item: torch.Tensor, mask: torch.Tensor, simi_pow: float, want_weights: bool = False):
    """MIND's label-aware attention (mind.py:303-333): user_emb_b = sum_k w_k I_bk with w = softmax over the valid capsules of
    simi_pow <I_bk, v_b>, v = the first B rows of `item` [M, D].  One launch each way, unless FUSED_LABEL_ATTENTION is off or
    `label_attention_ok` refuses the shape: then the literal form runs.  want_weights: -> (user_emb, w [B, K])."""
    if FUSED_LABEL_ATTENTION and label_attention_ok(interests, item, mask, simi_pow):
        out, w = _LabelAttentionFn.apply(interests, item, mask, float(simi_pow))
    else:
        out = label_attention_literal(interests, item, mask, float(simi_pow))
        w = None
        if want_weights:
            a = torch.einsum("bkd, bd->bk", interests, item[:interests.size(0)]).detach()
            w = torch.softmax(torch.minimum(a, (mask.to(a.dtype) * 2 - 1) * float("inf")) * float(simi_pow), dim=1)
    return (out, w) if want_weights else out


FUSED_AMM_LOSS = True  # profiles/amm_loss: the fused form against the literal one, without and with sample weights


def _div_no_nan(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    return torch.where(den != 0, num / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(num))


def _literal_grads(losses, gouts, inputs, needs, allow_unused: bool = False) -> tuple:
    """the backward of a fused loss that is asked for a double backward (create_graph): the gradients of sum(loss * gout) over the
    literal form's `losses` to the `inputs` that `needs` marks, None for the others, themselves differentiable"""
    total = sum(l * g for l, g in zip(losses, gouts) if g is not None)
    wanted = [t for t, need in zip(inputs, needs) if need]
    got = iter(torch.autograd.grad(total, wanted, create_graph=True, allow_unused=allow_unused))
    return tuple(next(got) if need else None for need in needs)


def amm_terms(user_augment: torch.Tensor, item_augment: torch.Tensor, user_tower_emb: torch.Tensor, item_tower_emb: torch.Tensor,
              c_u: float, c_i: float, weights: Optional[torch.Tensor] = None):
    """tzrec/models/dat.py:225-255, word for word, on the embeddings as the reference's towers deliver them (detached, normalized
    under COSINE) -> (amm_loss_u, amm_loss_i)"""
    batch_size = user_augment.size(0)
    dim = 1 if weights is not None else (0, 1)
    amm_loss_u = c_u * torch.sum(torch.square(F.normalize(user_augment, p=2.0, dim=1) - item_tower_emb[:batch_size]), dim=dim)
    amm_loss_i = c_i * torch.sum(torch.square(F.normalize(item_augment[:batch_size], p=2.0, dim=1) - user_tower_emb), dim=dim)
    if weights is not None:
        amm_loss_u = _div_no_nan(torch.mean(amm_loss_u * weights), torch.mean(weights))
        amm_loss_i = _div_no_nan(torch.mean(amm_loss_i * weights), torch.mean(weights))
    return amm_loss_u, amm_loss_i


def amm_loss_literal(user_aug, item_aug, user_emb, item_emb, cosine: bool, c_u: float, c_i: float, weights=None):
    """the towers' raw embeddings detached and, under COSINE, normalized as the reference's towers do before they return
    (dat.py:100-101, 206-207); then `amm_terms`"""
    user_emb, item_emb = user_emb.detach(), item_emb.detach()
    if cosine:
        user_emb, item_emb = F.normalize(user_emb, p=2.0, dim=1), F.normalize(item_emb, p=2.0, dim=1)
    return amm_terms(user_aug, item_aug, user_emb, item_emb, c_u, c_i, weights)


def amm_loss_ok(user_aug: torch.Tensor, item_aug: torch.Tensor, user_emb: torch.Tensor, item_emb: torch.Tensor,
                weights: Optional[torch.Tensor] = None) -> bool:
    """what tzr_amm_loss_* takes: fp32 user_aug / user_emb [B, D] and item_aug / item_emb [M >= B, D] with unit column stride, row
    strides that are multiples of 4 floats and 16-byte aligned rows (column slices of wider buffers are fine); D % 4 == 0, 4 <= D
    <= 256; B >= 1; weights fp32 [B] contiguous; everything on the device of the loaded library"""
    if any(t.dim() != 2 for t in (user_aug, item_aug, user_emb, item_emb)):
        return False
    B, D = user_aug.shape
    M = item_aug.shape[0]
    dev = user_aug.device
    if not _lib.takes(dev) or any(t.device != dev for t in (item_aug, user_emb, item_emb)):
        return False
    if not (D % 4 == 0 and 4 <= D <= _lib.AMM_MAX_D and B >= 1 and M >= B and user_emb.shape[0] == B and item_emb.shape[0] == M):
        return False
    if not all(_lib.rows_ok(t, D) for t in (user_aug, item_aug, user_emb, item_emb)):
        return False
    return weights is None or _lib.packed_ok(weights, (B,), dev)


class _AmmLossFn(torch.autograd.Function):
    """Inputs: user_aug [B, D], item_aug [M, D] (the gradients go here), user_emb [B, D], item_emb [M, D], weights [B] or None
    (constants).  Outputs: loss_u, loss_i (scalars).  Saved for the backward: the inputs and 6 B + 1 floats.  Capturable: the
    upstream gradients are read from device memory, every buffer is torch's.  Asked for a double backward, the backward
    differentiates the literal form instead."""

    @staticmethod
    def _fill(m, user_aug, item_aug, user_emb, item_emb, weights, cosine, c_u, c_i, rows, scale):
        m.B, m.M, m.D, m.cosine, m.c_u, m.c_i = user_aug.shape[0], item_aug.shape[0], user_aug.shape[1], int(cosine), c_u, c_i
        m.ua, m.ua_stride, m.ia, m.ia_stride = _lib.ptr(user_aug), user_aug.stride(0), _lib.ptr(item_aug), item_aug.stride(0)
        m.ue, m.ue_stride, m.ie, m.ie_stride = _lib.ptr(user_emb), user_emb.stride(0), _lib.ptr(item_emb), item_emb.stride(0)
        m.w = _lib.opt_ptr(weights)
        m.rows, m.scale = _lib.ptr(rows), _lib.ptr(scale)

    @staticmethod
    def forward(ctx, user_aug, item_aug, user_emb, item_emb, weights, cosine, c_u, c_i):
        B, dev = user_aug.shape[0], user_aug.device
        f32 = dict(dtype=torch.float32, device=dev)
        loss, rows, scale = torch.empty(2, **f32), torch.empty(6, B, **f32), torch.empty(1, **f32)
        m = _lib.TzrAmmLoss()
        _AmmLossFn._fill(m, user_aug, item_aug, user_emb, item_emb, weights, cosine, c_u, c_i, rows, scale)
        m.loss = _lib.ptr(loss)
        _lib.launch_ws("tzr_amm_loss", m, dev, "tzr_amm_loss_fwd")
        ctx.save_for_backward(user_aug, item_aug, user_emb, item_emb, weights, rows, scale)
        ctx.cfg = (cosine, c_u, c_i)
        ctx.set_materialize_grads(False)  # (no zero-filled gradient for a side nobody reads: a launch)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_u, g_i):
        user_aug, item_aug, user_emb, item_emb, weights, rows, scale = ctx.saved_tensors
        cosine, c_u, c_i = ctx.cfg
        none = (None,) * 6
        if g_u is None and g_i is None:
            return (None, None) + none
        if torch.is_grad_enabled():  # (create_graph: a double backward is coming)
            losses = amm_loss_literal(user_aug, item_aug, user_emb, item_emb, cosine, c_u, c_i, weights)
            return _literal_grads(losses, (g_u, g_i), (user_aug, item_aug), ctx.needs_input_grad[:2]) + none
        dev = user_aug.device
        g_u, g_i = (None if g is None else g.to(torch.float32) for g in (g_u, g_i))
        dua = torch.empty(user_aug.shape, dtype=torch.float32, device=dev)
        dia = torch.empty(item_aug.shape, dtype=torch.float32, device=dev)
        m = _lib.TzrAmmLoss()
        _AmmLossFn._fill(m, user_aug, item_aug, user_emb, item_emb, weights, cosine, c_u, c_i, rows, scale)
        m.grad_u, m.grad_i = _lib.opt_ptr(g_u), _lib.opt_ptr(g_i)
        m.dua, m.dua_stride, m.dia, m.dia_stride = _lib.ptr(dua), dua.stride(0), _lib.ptr(dia), dia.stride(0)
        _lib.launch("tzr_amm_loss_bwd", m, dev)
        return (dua, dia) + none


def amm_loss(user_aug: torch.Tensor, item_aug: torch.Tensor, user_emb: torch.Tensor, item_emb: torch.Tensor, cosine: bool,
             c_u: float, c_i: float, weights: Optional[torch.Tensor] = None):
    """DAT's Adaptive-Mimic loss -> (loss_u, loss_i).  user_aug [B, D] / item_aug [M >= B, D]: the towers' augment rows; user_emb
    [B, D] / item_emb [M, D]: the towers' embeddings before any normalisation, treated as detached.  loss_u = c_u sum_b |normalize(
    user_aug_b) - tau(item_emb_b)|^2 and loss_i likewise with the sides swapped, tau = normalize under `cosine`; with `weights` [B]:
    c mean(l w) / mean(w), 0 where mean(w) is 0.  Gradients go to the two augment tensors only.  One launch and a finishing one
    forward, one backward, unless FUSED_AMM_LOSS is off or `amm_loss_ok` refuses the operands: then the literal form runs."""
    if weights is not None:
        weights = weights.detach()
    user_emb, item_emb = user_emb.detach(), item_emb.detach()
    if FUSED_AMM_LOSS and amm_loss_ok(user_aug, item_aug, user_emb, item_emb, weights):
        return _AmmLossFn.apply(user_aug, item_aug, user_emb, item_emb, weights, bool(cosine), float(c_u), float(c_i))
    return amm_loss_literal(user_aug, item_aug, user_emb, item_emb, bool(cosine), float(c_u), float(c_i), weights)


NEG_DATA_GROUP = "__NEG__"  # tzrec/datasets/utils.py:29: the item-side features the negative sampler delivers, B + N rows


class MatchTower(nn.Module):
    """Base match tower (tzrec/models/match_model.py:110-199): one feature group, named by the tower block's `input` (MIND's user
    tower: that one and its history group), behind an EmbeddingGroup of its own over those groups' features."""

    def __init__(self, tower_config, output_dim: int, similarity: str, feature_group, features, device=None, sparse_optimizer=None,
                 batch_size: int = 1024, data_group: str = BASE_DATA_GROUP) -> None:
        super().__init__()
        self._group_name = str(tower_config.one("input"))
        self._output_dim, self._similarity = int(output_dim), similarity
        groups = list(feature_group) if isinstance(feature_group, (list, tuple)) else [feature_group]
        self.embedding_group = EmbeddingGroup(features, groups, device=device, sparse_optimizer=sparse_optimizer,
                                              batch_size=batch_size, data_group=data_group)

    def build_input(self, batch: Batch) -> Dict[str, torch.Tensor]:
        return self.embedding_group(batch)


class DSSMTower(MatchTower):
    """DSSM user / item tower (tzrec/models/dssm.py:38-83): `mlp` over the group, then `output` = Linear(., output_dim) when
    output_dim > 0.  The tower returns its embedding BEFORE the COSINE normalisation: that belongs to the similarity head
    (`match_softmax`), fused or literal."""

    def __init__(self, tower_config, output_dim: int, similarity: str, feature_group, features, device=None, sparse_optimizer=None,
                 batch_size: int = 1024, data_group: str = BASE_DATA_GROUP) -> None:
        super().__init__(tower_config, output_dim, similarity, feature_group, features, device, sparse_optimizer, batch_size, data_group)
        self._build_dense(self.embedding_group.group_total_dim(self._group_name), tower_config, device)

    def _build_dense(self, d_in: int, tower_config, device=None) -> None:
        from .rank_model import mlp_from_msg

        self.mlp = mlp_from_msg(d_in, tower_config.one("mlp"))
        if self._output_dim > 0:
            self.output = nn.Linear(self.mlp.output_dim(), self._output_dim)
        if device is not None:
            self.mlp.to(device)
            if self._output_dim > 0:
                self.output.to(device)

    def embedding_dim(self) -> int:
        return self._output_dim if self._output_dim > 0 else self.mlp.output_dim()

    def embed(self, x: torch.Tensor) -> torch.Tensor:
        """the group's features [rows, d_in] -> the tower's embedding"""
        out = self.mlp(x)
        if self._output_dim > 0:
            out = self.output(out)
        return out

    def forward(self, batch: Batch) -> torch.Tensor:
        return self.embed(self.build_input(batch)[self._group_name])


class ConfigMatchModel(nn.Module):
    """What the config-built match models share (tzrec/models/match_model.py:246-336): the refusals, the two towers' feature
    groups and features, the similarity head and the plumbing the pipelines read.  A subclass names its block (`_NAME`), the
    block's and the towers' fields, the default similarity, and builds `user_tower` / `item_tower` in `_build_towers`;
    `_embeddings(batch)` hands the head its user [B, D] and item [M, D] rows, `_head_cosine` says whether the head still
    normalizes them."""

    _NAME = ""
    _FIELDS: tuple = ()
    _TOWER_FIELDS: Dict[str, tuple] = {}
    _TOWER_GROUPS: Dict[str, tuple] = {"user_tower": ("input",), "item_tower": ("input",)}  # the tower fields that name a feature group
    _DEFAULT_SIMILARITY = "INNER_PRODUCT"

    def __init__(self, spec, device=None, sparse_optimizer=None) -> None:
        super().__init__()
        from .rank_model import RankModel

        name, m = self._NAME, spec.model
        if RankModel._build_pg is not None:
            raise NotImplementedError(f"{name}: `process_group` (sharded towers) is not built")
        other = sorted(k for k in m if k not in self._FIELDS)
        if other:
            raise ValueError(f"{name}: {name} has no field {other[0]!r} (fields: {', '.join(self._FIELDS)})")
        for k in spec.sampler_kinds:
            if k != "negative_sampler":
                raise NotImplementedError(f"{name}: data_config `{k}` is not built (built: negative_sampler)")
        for k in ("variational_dropout", "train_metrics"):
            if k in spec.model_config_keys:
                raise NotImplementedError(f"{name}: model_config `{k}` is not built")
        if len(spec.losses) != 1 or spec.losses[0].kind != "softmax_cross_entropy":
            raise ValueError(f"{name}: a match model takes exactly one loss, softmax_cross_entropy (got {[l.kind for l in spec.losses]})")
        if float(spec.losses[0].fields.get("label_smoothing", 0.0)) != 0.0:
            raise NotImplementedError(f"{name}: softmax_cross_entropy `label_smoothing` is not built for match models")
        for ms in spec.metrics:
            if ms.kind != "recall_at_k":
                raise ValueError(f"{name}: a match model's metrics are recall_at_k only (got {ms.kind!r})")
        self._in_batch = bool(m.one("in_batch_negative", False))
        self._sampler = spec.negative_sampler
        if self._in_batch and self._sampler is not None:
            raise ValueError(f"{name}: `in_batch_negative: true` together with a negative_sampler is not built (the reference adds "
                             "the in-batch columns to the sampled ones)")
        for k in ("user_tower", "item_tower", "output_dim"):
            if not m.has(k):
                raise ValueError(f"{name}: needs `{k}`")
        similarity = str(m.one("similarity", self._DEFAULT_SIMILARITY)).upper()
        if similarity not in ("INNER_PRODUCT", "COSINE"):
            raise ValueError(f"{name}: similarity {similarity!r} (INNER_PRODUCT, COSINE)")
        self._cosine, self._temperature = similarity == "COSINE", float(m.one("temperature", 1.0))
        self._mode = IN_BATCH if self._in_batch else SAMPLED
        self._spec, self._pg = spec, None
        self._weight = spec.sample_weight_fields[0] if spec.sample_weight_fields else None
        self.want_similarity = False
        groups = {g.group_name: g for g in spec.feature_groups}
        by_name = {f.name: f for f in spec.features}
        towers, tables = {}, {}
        for which in ("user_tower", "item_tower"):
            t = m.one(which)
            other = sorted(k for k in t if k not in self._TOWER_FIELDS[which])
            if other:
                raise ValueError(f"{name}: {which} has no field {other[0]!r} (fields: {', '.join(self._TOWER_FIELDS[which])})")
            gs, feats = [], []
            for field in self._TOWER_GROUPS[which]:
                if not t.has(field):
                    raise ValueError(f"{name}: {which} needs `{field}`")
                gname = str(t.one(field))
                if gname not in groups:
                    raise ValueError(f"{name}: {which}.{field} {gname!r} is not a feature group of the config")
                g = groups[gname]
                gs.append(g)
                feats += list(g.feature_names) + [n for sg in g.sequence_groups for n in sg.feature_names]
            feats = [by_name[n] for n in dict.fromkeys(feats) if n in by_name]
            for f in feats:
                if f.zch is not None:
                    raise NotImplementedError(f"{name}: {which}: feature {f.name!r} has a zero-collision hash (`zch`): not built in a match tower")
            tables[which] = {f.embedding_name or f"{f.name}_emb" for f in feats if f.is_sparse}
            towers[which] = (t, gs, feats)
        shared = sorted(tables["user_tower"] & tables["item_tower"])
        if shared:
            raise NotImplementedError(f"{name}: table {shared[0]!r} appears in both towers' groups: each tower owns its tables")
        so = sparse_optimizer if sparse_optimizer is not None else spec.sparse_optimizer
        self._build_towers(towers, int(m.one("output_dim")), similarity, device, so, spec.batch_size or 1024,
                           NEG_DATA_GROUP if self._sampler is not None else BASE_DATA_GROUP)

    def _build_towers(self, towers, out_dim: int, similarity: str, device, sparse_optimizer, batch_size: int, item_data_group: str) -> None:
        raise NotImplementedError

    @property
    def _head_cosine(self) -> bool:
        """whether the similarity head normalizes the embeddings it is handed"""
        return self._cosine

    # ---- what the pipelines and the example read
    def dense_parameters(self):
        for n, p in self.named_parameters():
            if not n.startswith(("user_tower.embedding_group.", "item_tower.embedding_group.")):
                yield p

    @property
    def fused_optimizers(self):
        return [fo for fo in (self.user_tower.embedding_group.fused_optimizer, self.item_tower.embedding_group.fused_optimizer) if fo is not None]

    def sync_dense_parameters(self) -> None:
        """(single process: nothing to broadcast; sharded towers are refused when the model is built)"""

    def allreduce_dense_grads(self) -> None:
        return

    def _embeddings(self, batch: Batch):
        return self.user_tower(batch), self.item_tower(batch)

    def _weights(self, batch: Batch):
        return batch.sample_weights[self._weight].to(torch.float32) if self._weight else None

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        """{"similarity": [B, 1 + N] or [B, B], "rank": [B]}: the scores materialised, differentiable (the literal form) under
        autograd, out of the fused forward under no_grad (evaluation)"""
        u, v = self._embeddings(batch)
        if not torch.is_grad_enabled():
            _, rank, sim = match_softmax(u, v, self._mode, self._head_cosine, self._temperature, None, want_sim=True)
            return {"similarity": sim, "rank": rank}
        sim = match_scores(u, v, self._mode, self._head_cosine, self._temperature)
        return {"similarity": sim, "rank": scores_loss_rank(sim.detach(), self._mode)[1]}

    def loss(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        return {"softmax_cross_entropy": scores_loss_rank(predictions["similarity"], self._mode, self._weights(batch))[0]}

    def head(self, u: torch.Tensor, v: torch.Tensor, weights: Optional[torch.Tensor] = None):
        """the towers' embeddings -> ({"softmax_cross_entropy": loss}, {"rank": rank[, "similarity": sim]}) on the fused head"""
        loss, rank, sim = match_softmax(u, v, self._mode, self._head_cosine, self._temperature, weights, want_sim=self.want_similarity)
        predictions = {"rank": rank}
        if sim is not None:
            predictions["similarity"] = sim
        return {"softmax_cross_entropy": loss}, predictions

    def loss_and_predictions(self, batch: Batch):
        u, v = self._embeddings(batch)
        return self.head(u, v, self._weights(batch))


class ConfigDSSM(ConfigMatchModel):
    """`dssm { user_tower {} item_tower {} output_dim similarity temperature in_batch_negative }` (tzrec/models/dssm.py:86-155,
    match_model.py:246-336): two DSSMTowers, each with the EmbeddingGroup of its own feature group, and the similarity head.

    With `data_config.negative_sampler` the item tower reads the batch's "__NEG__" data group: B + num_sample rows, row i the
    positive of user row i, the rest negatives shared by the batch; with `in_batch_negative` it reads the base group's B rows and
    every other row of the batch is a negative.  Without either the positive is the only column (loss 0), as in the reference.

    `loss_and_predictions(batch)` -- what the train pipelines call -- runs the fused head: {"softmax_cross_entropy": loss} and
    {"rank": rank} (plus "similarity" when `want_similarity` is set), no score matrix otherwise.  `forward(batch)` keeps the
    literal contract, {"similarity": [B, C]} (plus "rank"), for `loss(predictions, batch)` and evaluation.

    Refused when built, by name: every sampler but `negative_sampler`; `variational_dropout`; `train_metrics`; any loss but one
    `softmax_cross_entropy`; any metric but `recall_at_k` (both the reference's own assertions, match_model.py:284-291, 345-348);
    `in_batch_negative` with a sampler; a table that both towers' groups would share; a zero-collision-hash feature; sharded
    towers (`process_group`); a field the `dssm` block or a tower block does not have."""

    _NAME = "dssm"
    _FIELDS = ("user_tower", "item_tower", "output_dim", "similarity", "temperature", "in_batch_negative")
    _TOWER_FIELDS = {"user_tower": ("input", "mlp"), "item_tower": ("input", "mlp")}

    def _build_towers(self, towers, out_dim, similarity, device, sparse_optimizer, batch_size, item_data_group) -> None:
        t, gs, feats = towers["user_tower"]
        self.user_tower = DSSMTower(t, out_dim, similarity, gs[0], feats, device, sparse_optimizer, batch_size)
        t, gs, feats = towers["item_tower"]
        self.item_tower = DSSMTower(t, out_dim, similarity, gs[0], feats, device, sparse_optimizer, batch_size, data_group=item_data_group)
        if self.user_tower.embedding_dim() != self.item_tower.embedding_dim():
            raise ValueError(f"dssm: the towers end {self.user_tower.embedding_dim()} and {self.item_tower.embedding_dim()} wide")


class DATTower(DSSMTower):
    """DAT user / item tower (tzrec/models/dat.py:39-106): one EmbeddingGroup over the `input` group and the `augment_input`
    group; `mlp` over cat([input group, augment group], 1), then `output`.  -> (embedding, augment rows): the embedding BEFORE the
    COSINE normalisation, as DSSMTower's, the augment group's rows as the embedding group delivers them."""

    def __init__(self, tower_config, output_dim: int, similarity: str, feature_groups, features, device=None, sparse_optimizer=None,
                 batch_size: int = 1024, data_group: str = BASE_DATA_GROUP) -> None:
        MatchTower.__init__(self, tower_config, output_dim, similarity, list(feature_groups), features, device, sparse_optimizer,
                            batch_size, data_group)
        self._augment_group_name = str(tower_config.one("augment_input"))
        eg = self.embedding_group
        self._build_dense(eg.group_total_dim(self._group_name) + eg.group_total_dim(self._augment_group_name), tower_config, device)

    def augment_dim(self) -> int:
        return self.embedding_group.group_total_dim(self._augment_group_name)

    def forward(self, batch: Batch):
        feats = self.build_input(batch)
        augment = feats[self._augment_group_name]
        return self.embed(torch.cat([feats[self._group_name], augment], dim=1)), augment


class ConfigDAT(ConfigMatchModel):
    """`dat { user_tower {} item_tower {} output_dim similarity temperature in_batch_negative amm_i_weight amm_u_weight }`
    (tzrec/models/dat.py, protos/models/match_model.proto: DAT, protos/tower.proto: DATTower): two DATTowers, each reading a second
    "augment" feature group next to its own, DSSM's similarity head, and in training the Adaptive-Mimic loss that pulls each
    tower's normalized augment rows towards the other tower's detached embedding of the same sample (`amm_loss`).  A feature may
    sit in a tower's group and in its augment group (the docs' user_id / item_id): one lookup, copied into both, gradient from both.

    `loss_and_predictions(batch)`: {"softmax_cross_entropy"} from the fused head plus, in training mode, {"amm_loss_u",
    "amm_loss_i"}; under `eval()` the first alone, as the reference's towers return no augment vector then.  `forward(batch)`
    keeps the literal contract: under autograd in training mode "similarity", "rank", "user_augment", "item_augment" and the
    detached "user_tower_emb" / "item_tower_emb" (normalized under COSINE), from which `loss(predictions, batch)` computes the
    literal terms; under no_grad or `eval()` "similarity" and "rank" alone.  With a negative sampler the item tower reads
    "__NEG__" (B + N rows) and the AMM terms use its first B rows.

    Refused when built, by name: everything ConfigDSSM refuses; a missing `amm_i_weight` / `amm_u_weight` (`required` in the
    proto); a tower without `augment_input`; an augment group that is not a DEEP group of the config; an augment group whose total
    dim differs from the towers' embedding dim (the reference would fail at the subtraction, or silently broadcast a 1-wide
    group); towers ending in different widths."""

    _NAME = "dat"
    _FIELDS = ("user_tower", "item_tower", "output_dim", "similarity", "temperature", "in_batch_negative", "amm_i_weight", "amm_u_weight")
    _TOWER_FIELDS = {"user_tower": ("input", "augment_input", "mlp"), "item_tower": ("input", "augment_input", "mlp")}
    _TOWER_GROUPS = {"user_tower": ("input", "augment_input"), "item_tower": ("input", "augment_input")}

    def _build_towers(self, towers, out_dim, similarity, device, sparse_optimizer, batch_size, item_data_group) -> None:
        m = self._spec.model
        for k in ("amm_i_weight", "amm_u_weight"):
            if not m.has(k):
                raise ValueError(f"dat: needs `{k}` (required in the proto)")
        self._amm_u, self._amm_i = float(m.one("amm_u_weight")), float(m.one("amm_i_weight"))
        for which in ("user_tower", "item_tower"):
            for field, g in zip(self._TOWER_GROUPS[which], towers[which][1]):
                if g.group_type != "DEEP":
                    raise ValueError(f"dat: {which}.{field} {g.group_name!r} is a {g.group_type} group: the towers read DEEP groups")
        t, gs, feats = towers["user_tower"]
        self.user_tower = DATTower(t, out_dim, similarity, gs, feats, device, sparse_optimizer, batch_size)
        t, gs, feats = towers["item_tower"]
        self.item_tower = DATTower(t, out_dim, similarity, gs, feats, device, sparse_optimizer, batch_size, data_group=item_data_group)
        if self.user_tower.embedding_dim() != self.item_tower.embedding_dim():
            raise ValueError(f"dat: the towers end {self.user_tower.embedding_dim()} and {self.item_tower.embedding_dim()} wide")
        for which, tower in (("user_tower", self.user_tower), ("item_tower", self.item_tower)):
            if tower.augment_dim() != tower.embedding_dim():
                raise ValueError(f"dat: {which}.augment_input {tower._augment_group_name!r} is {tower.augment_dim()} wide, the towers' "
                                 f"embedding {tower.embedding_dim()}: the Adaptive-Mimic loss subtracts one from the other")

    def _embeddings(self, batch: Batch):
        return self.user_tower(batch)[0], self.item_tower(batch)[0]

    def forward(self, batch: Batch) -> Dict[str, torch.Tensor]:
        if not (self.training and torch.is_grad_enabled()):
            return super().forward(batch)
        (u, user_augment), (v, item_augment) = self.user_tower(batch), self.item_tower(batch)
        sim = match_scores(u, v, self._mode, self._head_cosine, self._temperature)
        ue, ve = u.detach(), v.detach()
        if self._cosine:
            ue, ve = F.normalize(ue, p=2.0, dim=1), F.normalize(ve, p=2.0, dim=1)
        return {"similarity": sim, "rank": scores_loss_rank(sim.detach(), self._mode)[1], "user_augment": user_augment,
                "item_augment": item_augment, "user_tower_emb": ue, "item_tower_emb": ve}

    def loss(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        losses = super().loss(predictions, batch)
        if "user_augment" in predictions:
            losses["amm_loss_u"], losses["amm_loss_i"] = amm_terms(predictions["user_augment"], predictions["item_augment"],
                                                                   predictions["user_tower_emb"], predictions["item_tower_emb"],
                                                                   self._amm_u, self._amm_i, self._weights(batch))
        return losses

    def loss_and_predictions(self, batch: Batch):
        if not self.training:
            return super().loss_and_predictions(batch)
        (u, user_augment), (v, item_augment) = self.user_tower(batch), self.item_tower(batch)
        weights = self._weights(batch)
        losses, predictions = self.head(u, v, weights)
        losses["amm_loss_u"], losses["amm_loss_i"] = amm_loss(user_augment, item_augment, u, v, self._cosine, self._amm_u, self._amm_i, weights)
        return losses, predictions


_CAPSULE_FIELDS = ("max_k", "max_seq_len", "high_dim", "num_iters", "routing_logits_scale", "routing_logits_stddev", "squash_pow",
                   "const_caps_num", "routing_init_method")


def capsule_config_from_msg(msg) -> CapsuleConfig:
    """a `capsule_config { }` block (protos/module.proto: B2ICapsule) with the reference's defaults"""
    other = sorted(k for k in msg if k not in _CAPSULE_FIELDS)
    if other:
        raise ValueError(f"mind: capsule_config has no field {other[0]!r} (fields: {', '.join(_CAPSULE_FIELDS)})")
    for k in ("max_seq_len", "high_dim"):
        if not msg.has(k):
            raise ValueError(f"mind: capsule_config needs `{k}`")
    init = str(msg.one("routing_init_method", "normal"))
    if init not in ("normal", "zeros"):
        raise ValueError(f"mind: capsule_config.routing_init_method {init!r}: init_method should be 'normal' or 'zeros'")
    return CapsuleConfig(max_k=int(msg.one("max_k", 5)), max_seq_len=int(msg.one("max_seq_len")), high_dim=int(msg.one("high_dim")),
                         num_iters=int(msg.one("num_iters", 3)), routing_logits_scale=float(msg.one("routing_logits_scale", 20.0)),
                         routing_logits_stddev=float(msg.one("routing_logits_stddev", 1.0)), squash_pow=float(msg.one("squash_pow", 1.0)),
                         const_caps_num=bool(msg.one("const_caps_num", False)), routing_init_method=init)


class MINDUserTower(MatchTower):
    """MIND's user tower (tzrec/models/mind.py:30-194) with the reference's parameter names: `user_mlp` (all but the last of
    user_mlp.hidden_units) and `user_mlp_out` over the user group; `_hist_seq_mlp` / `_hist_seq_mlp_out` (no bias) over the
    history; `_capsule_layer`; `_concat_mlp` over [user feature | interest] per interest; `output` = Linear(., output_dim) without
    bias.  -> (interests [B, max_k, D], capsule mask [B, max_k]), the interests normalized under COSINE.

    The history group is read as ROWS (`<g>.sequence_jagged` / `<g>.sequence_offsets` of the embedding group) whenever its features
    are the sub-features of one `sequence_feature` block with a `sequence_length`: `_hist_seq_mlp` runs on the [N, D] rows -- exact,
    it has no bias and the capsule layer masks its input -- and the capsule layer on the rows (capsule.capsule_routing).  Any other
    history group is read padded and its valid positions are gathered into rows (a device read-back: not capturable).
    `_concat_mlp` runs on the [B max_k, .] rows.  `user_seq_combine` is accepted and has no effect, as in the reference, which
    never reads it."""

    def __init__(self, tower_config, output_dim: int, similarity: str, user_group, hist_group, features, device=None, sparse_optimizer=None,
                 batch_size: int = 1024) -> None:
        super().__init__(tower_config, output_dim, similarity, [user_group, hist_group], features, device, sparse_optimizer, batch_size)
        self._hist_group_name = hist_group.group_name
        eg = self.embedding_group
        info = eg._seq_info[self._hist_group_name]
        if info["max_len"] and len({f.name.split("__")[0] for f in info["sequence"]}) == 1 \
                and not any(getattr(f, "value_dim", 1) not in (0, 1) for f in info["sequence"]):
            eg.jagged_sequence_groups.add(self._hist_group_name)
        self._build_dense(eg.group_total_dim(self._group_name), eg.group_total_dim(self._hist_group_name + ".sequence"), tower_config, device)

    def _build_dense(self, d_user: int, d_hist: int, tower_config, device=None) -> None:
        from .dlrm import MLP
        from .rank_model import mlp_kwargs

        user = mlp_kwargs(tower_config.one("user_mlp"))
        if len(user["hidden_units"]) < 2:
            raise ValueError("mind: user_tower.user_mlp needs at least two hidden_units (the reference itself fails with fewer, mind.py:83-85)")
        first = lambda d: d[0] if d else None  # noqa: E731  (the reference hands the MLP dropout_ratio[0])
        self.user_mlp = MLP(d_user, user["hidden_units"][:-1], activation=user["activation"], use_bn=user["use_bn"],
                            dropout_ratio=first(user["dropout_ratio"]))
        self.user_mlp_out = nn.Linear(self.user_mlp.output_dim(), user["hidden_units"][-1])
        self._hist_seq_mlp = self._hist_seq_mlp_out = None
        hist = mlp_kwargs(tower_config.one("hist_seq_mlp")) if tower_config.has("hist_seq_mlp") else None
        for which, kw in (("hist_seq_mlp", hist), ("concat_mlp", mlp_kwargs(tower_config.one("concat_mlp")))):
            if kw is not None and kw["use_bn"]:
                raise NotImplementedError(f"mind: user_tower.{which} `use_bn` is not built (batch statistics over padded positions "
                                          "cannot be restated on rows)")
        if hist is not None and len(hist["hidden_units"]) > 1:
            self._hist_seq_mlp = MLP(d_hist, hist["hidden_units"][:-1], bias=False, activation=hist["activation"], dropout_ratio=first(hist["dropout_ratio"]))
            self._hist_seq_mlp_out = nn.Linear(self._hist_seq_mlp.output_dim(), hist["hidden_units"][-1], bias=False)
            d_hist = hist["hidden_units"][-1]
        elif hist is not None and len(hist["hidden_units"]) > 0:
            self._hist_seq_mlp = nn.Linear(d_hist, hist["hidden_units"][-1], bias=False)
            d_hist = hist["hidden_units"][-1]
        cfg = capsule_config_from_msg(tower_config.one("capsule_config"))
        self._capsule_layer = CapsuleLayer(cfg, d_hist)
        self._concat_mlp = MLP(user["hidden_units"][-1] + cfg.high_dim, **mlp_kwargs(tower_config.one("concat_mlp")))
        if self._output_dim > 0:
            self.output = nn.Linear(self._concat_mlp.output_dim(), self._output_dim, bias=False)
        if device is not None:
            for name, mod in self.named_children():
                if name != "embedding_group":
                    mod.to(device)

    def embedding_dim(self) -> int:
        return self._output_dim if self._output_dim > 0 else self._concat_mlp.output_dim()

    def history_rows(self, feats: Dict[str, torch.Tensor]):
        """-> (rows [N, D], offsets [B + 1]) of the history group"""
        g = self._hist_group_name
        if g in self.embedding_group.jagged_sequence_groups:
            return feats[f"{g}.sequence_jagged"], feats[f"{g}.sequence_offsets"]
        seq, lens = feats[f"{g}.sequence"], feats[f"{g}.sequence_length"].clamp(max=feats[f"{g}.sequence"].shape[1])
        keep = torch.arange(seq.shape[1], device=seq.device)[None, :] < lens[:, None]
        return seq[keep], torch.cat([lens.new_zeros(1), lens.cumsum(0)])

    def interests(self, user_x: torch.Tensor, rows: torch.Tensor, offsets: torch.Tensor, logits0: Optional[torch.Tensor] = None):
        """the user group's features [B, .] and the history rows -> (interests [B, K, D], mask [B, K]) (mind.py:158-194); logits0
        [N, K]: the capsule layer's initial routing logits instead of its own draw"""
        user_feature = self.user_mlp_out(self.user_mlp(user_x))
        if self._hist_seq_mlp is not None:
            rows = self._hist_seq_mlp(rows)
            if self._hist_seq_mlp_out is not None:
                rows = self._hist_seq_mlp_out(rows)
        high, mask = self._capsule_layer(rows, offsets, logits0)
        B, K, _ = high.shape
        maskf = mask.unsqueeze(-1).to(high.dtype)
        x = torch.cat([user_feature.unsqueeze(1).expand(B, K, user_feature.shape[1]), high], dim=-1) * maskf
        x = self._concat_mlp(x.reshape(B * K, -1)).reshape(B, K, -1) * maskf
        if self._output_dim > 0:
            x = self.output(x)
        if self._similarity == "COSINE":
            x = F.normalize(x, p=2.0, dim=-1)
        return x, mask

    def forward(self, batch: Batch):
        feats = self.build_input(batch)
        rows, offsets = self.history_rows(feats)
        return self.interests(feats[self._group_name], rows, offsets)


class MINDItemTower(DSSMTower):
    """MIND's item tower (mind.py:197-252): DSSM's, plus its own normalisation under COSINE"""

    def embed(self, x: torch.Tensor) -> torch.Tensor:
        out = super().embed(x)
        return F.normalize(out, p=2.0, dim=1) if self._similarity == "COSINE" else out


class ConfigMIND(ConfigMatchModel):
    """`mind { user_tower {} item_tower {} simi_pow similarity in_batch_negative temperature output_dim }` (tzrec/models/mind.py,
    match_model.py:246-336): a MINDUserTower over the groups `input` and `history_input`, a MINDItemTower, the label-aware
    attention of the positive item over the user's interests (`label_attention`) and DSSM's similarity head.  The towers
    normalize under COSINE (the default here), so the head runs without its own normalisation; the attended user embedding is
    deliberately not re-normalized: the reference has that line commented out (mind.py:356-357).

    Data groups, `loss_and_predictions`, `forward`, `loss`, `head`: as ConfigDSSM.  Refused when built, by name: everything
    ConfigDSSM refuses (hard-negative samplers among it); `user_mlp` with fewer than two `hidden_units`; `use_bn` in `hist_seq_mlp`
    or `concat_mlp`; a field the `mind` block, a tower or `capsule_config` does not have; a `routing_init_method` other than
    normal / zeros; a `history_input` that is not a SEQUENCE group.  The inference form that returns the interests instead of one
    user embedding (mind.py:191-192) is not built: no method of this class returns them."""

    _NAME = "mind"
    _FIELDS = ("user_tower", "item_tower", "simi_pow", "similarity", "in_batch_negative", "temperature", "output_dim")
    _TOWER_FIELDS = {"user_tower": ("input", "history_input", "user_mlp", "hist_seq_mlp", "user_seq_combine", "capsule_config", "concat_mlp"),
                     "item_tower": ("input", "mlp")}
    _TOWER_GROUPS = {"user_tower": ("input", "history_input"), "item_tower": ("input",)}
    _DEFAULT_SIMILARITY = "COSINE"

    def _build_towers(self, towers, out_dim, similarity, device, sparse_optimizer, batch_size, item_data_group) -> None:
        t, gs, feats = towers["user_tower"]
        for k in ("user_mlp", "capsule_config", "concat_mlp"):
            if not t.has(k):
                raise ValueError(f"mind: user_tower needs `{k}`")
        if gs[1].group_type != "SEQUENCE":
            raise ValueError(f"mind: user_tower.history_input {gs[1].group_name!r} is a {gs[1].group_type} group: the history is a SEQUENCE group")
        if gs[0].group_type == "SEQUENCE":
            raise ValueError(f"mind: user_tower.input {gs[0].group_name!r} is a SEQUENCE group")
        self._simi_pow = float(self._spec.model.one("simi_pow", 10.0))
        self.user_tower = MINDUserTower(t, out_dim, similarity, gs[0], gs[1], feats, device, sparse_optimizer, batch_size)
        t, gs, feats = towers["item_tower"]
        self.item_tower = MINDItemTower(t, out_dim, similarity, gs[0], feats, device, sparse_optimizer, batch_size, data_group=item_data_group)
        if self.user_tower.embedding_dim() != self.item_tower.embedding_dim():
            raise ValueError(f"mind: the towers end {self.user_tower.embedding_dim()} and {self.item_tower.embedding_dim()} wide")

    @property
    def _head_cosine(self) -> bool:
        return False  # (the towers have normalized)

    def _embeddings(self, batch: Batch):
        interests, mask = self.user_tower(batch)
        v = self.item_tower(batch)
        return label_attention(interests, v, mask, self._simi_pow), v
