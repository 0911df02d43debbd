"""The match (retrieval) models: the fused similarity head and DSSM built from its config.

`match_softmax` is the head of tzrec/models/match_model.py:50-64, 303-336 and dssm.py:81-83, 147-155 -- normalize,
similarity, temperature, softmax cross entropy -- plus the rank of the positive that recall@k needs, in one autograd Function over
tzr_match_softmax_fwd / _bwd (csrc/match_softmax.hip): the [B, 1 + N] (or [B, B]) score matrix is never in memory unless the
caller asks for it.  `FUSED_MATCH_SOFTMAX = False`, or a shape outside `match_softmax_ok`, runs the reference's literal form.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .embedding_group import BASE_DATA_GROUP, Batch, EmbeddingGroup

SAMPLED, IN_BATCH = _lib.MATCH_SAMPLED, _lib.MATCH_IN_BATCH
FUSED_MATCH_SOFTMAX = True  # profiles/match_softmax: the fused head against the literal one at both modes' example shapes


def _rows_ok(x: torch.Tensor, D: int) -> bool:
    return bool(x.dim() == 2 and x.shape[1] == D and x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) % 4 == 0
                and x.stride(0) >= D and x.data_ptr() % 16 == 0)


def match_softmax_ok(user: torch.Tensor, item: torch.Tensor, mode: int, weights: Optional[torch.Tensor] = None) -> bool:
    """what tzr_match_softmax_* takes: fp32 user [B, D] and item [M, D] with unit column stride, row strides that are multiples of
    4 floats and 16-byte aligned rows (column slices of wider buffers are fine); D % 4 == 0, 4 <= D <= 256; B >= 1; M >= B in
    SAMPLED mode (N = M - B negatives, N = 0 allowed), M == B in IN_BATCH mode; weights fp32 [B] contiguous; everything on the
    device of the loaded library"""
    if user.dim() != 2 or item.dim() != 2:
        return False
    B, D = user.shape
    if (user.device.type == "cpu") != (_lib.backend() == "emu") or item.device != user.device:
        return False
    if not (D % 4 == 0 and 4 <= D <= _lib.MATCH_SOFTMAX_MAX_D and B >= 1 and _rows_ok(user, D) and _rows_ok(item, D)):
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
    if weights is not None and not (weights.shape == (B,) and weights.dtype == torch.float32 and weights.is_contiguous()
                                    and weights.device == user.device):
        return False
    return True


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
        m.w = _lib.ptr(weights) if weights is not None else 0
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
        L = _lib.lib()
        ws = _lib.workspace(L.tzr_match_softmax_workspace(C.byref(m)), dev)
        m.ws, m.ws_bytes = _lib.ptr(ws), ws.numel()
        _lib.check(L.tzr_match_softmax_fwd(C.byref(m), _lib.stream_ptr(dev)), "tzr_match_softmax_fwd")
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
        _lib.check(_lib.lib().tzr_match_softmax_bwd(C.byref(m), _lib.stream_ptr(dev)), "tzr_match_softmax_bwd")
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


NEG_DATA_GROUP = "__NEG__"  # tzrec/datasets/utils.py:29: the item-side features the negative sampler delivers, B + N rows


class MatchTower(nn.Module):
    """Base match tower (tzrec/models/match_model.py:110-199): one feature group, named by the tower block's `input`, behind an
    EmbeddingGroup of its own over that group's features."""

    def __init__(self, tower_config, output_dim: int, similarity: str, feature_group, features, device=None, sparse_optimizer=None,
                 batch_size: int = 1024, data_group: str = BASE_DATA_GROUP) -> None:
        super().__init__()
        self._group_name = str(tower_config.one("input"))
        self._output_dim, self._similarity = int(output_dim), similarity
        self.embedding_group = EmbeddingGroup(features, [feature_group], device=device, sparse_optimizer=sparse_optimizer,
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


class ConfigDSSM(nn.Module):
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

    _FIELDS = ("user_tower", "item_tower", "output_dim", "similarity", "temperature", "in_batch_negative")
    _TOWER_FIELDS = ("input", "mlp")

    def __init__(self, spec, device=None, sparse_optimizer=None) -> None:
        super().__init__()
        from .rank_model import RankModel

        m = spec.model
        if RankModel._build_pg is not None:
            raise NotImplementedError("dssm: `process_group` (sharded towers) is not built")
        other = sorted(k for k in m if k not in self._FIELDS)
        if other:
            raise ValueError(f"dssm: dssm has no field {other[0]!r} (fields: {', '.join(self._FIELDS)})")
        for k in spec.sampler_kinds:
            if k != "negative_sampler":
                raise NotImplementedError(f"dssm: data_config `{k}` is not built (built: negative_sampler)")
        for k in ("variational_dropout", "train_metrics"):
            if k in spec.model_config_keys:
                raise NotImplementedError(f"dssm: model_config `{k}` is not built")
        if len(spec.losses) != 1 or spec.losses[0].kind != "softmax_cross_entropy":
            raise ValueError(f"dssm: a match model takes exactly one loss, softmax_cross_entropy (got {[l.kind for l in spec.losses]})")
        if float(spec.losses[0].fields.get("label_smoothing", 0.0)) != 0.0:
            raise NotImplementedError("dssm: softmax_cross_entropy `label_smoothing` is not built for match models")
        for ms in spec.metrics:
            if ms.kind != "recall_at_k":
                raise ValueError(f"dssm: a match model's metrics are recall_at_k only (got {ms.kind!r})")
        self._in_batch = bool(m.one("in_batch_negative", False))
        self._sampler = spec.negative_sampler
        if self._in_batch and self._sampler is not None:
            raise ValueError("dssm: `in_batch_negative: true` together with a negative_sampler is not built (the reference adds "
                             "the in-batch columns to the sampled ones)")
        for k in ("user_tower", "item_tower", "output_dim"):
            if not m.has(k):
                raise ValueError(f"dssm: needs `{k}`")
        similarity = str(m.one("similarity", "INNER_PRODUCT")).upper()
        if similarity not in ("INNER_PRODUCT", "COSINE"):
            raise ValueError(f"dssm: similarity {similarity!r} (INNER_PRODUCT, COSINE)")
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
            other = sorted(k for k in t if k not in self._TOWER_FIELDS)
            if other:
                raise ValueError(f"dssm: {which} has no field {other[0]!r} (fields: {', '.join(self._TOWER_FIELDS)})")
            gname = str(t.one("input"))
            if gname not in groups:
                raise ValueError(f"dssm: {which}.input {gname!r} is not a feature group of the config")
            g = groups[gname]
            names = list(g.feature_names) + [n for sg in g.sequence_groups for n in sg.feature_names]
            feats = [by_name[n] for n in dict.fromkeys(names) if n in by_name]
            for f in feats:
                if f.zch is not None:
                    raise NotImplementedError(f"dssm: {which}: feature {f.name!r} has a zero-collision hash (`zch`): not built in a match tower")
            tables[which] = {f.embedding_name or f"{f.name}_emb" for f in feats if f.is_sparse}
            towers[which] = (t, g, feats)
        shared = sorted(tables["user_tower"] & tables["item_tower"])
        if shared:
            raise NotImplementedError(f"dssm: table {shared[0]!r} appears in both towers' groups: each tower owns its tables")
        out_dim = int(m.one("output_dim"))
        so = sparse_optimizer if sparse_optimizer is not None else spec.sparse_optimizer
        bs = spec.batch_size or 1024
        t, g, feats = towers["user_tower"]
        self.user_tower = DSSMTower(t, out_dim, similarity, g, feats, device, so, bs)
        t, g, feats = towers["item_tower"]
        self.item_tower = DSSMTower(t, out_dim, similarity, g, feats, device, so, bs,
                                    data_group=NEG_DATA_GROUP if self._sampler is not None else BASE_DATA_GROUP)
        if self.user_tower.embedding_dim() != self.item_tower.embedding_dim():
            raise ValueError(f"dssm: the towers end {self.user_tower.embedding_dim()} and {self.item_tower.embedding_dim()} wide")

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
            _, rank, sim = match_softmax(u, v, self._mode, self._cosine, self._temperature, None, want_sim=True)
            return {"similarity": sim, "rank": rank}
        sim = match_scores(u, v, self._mode, self._cosine, self._temperature)
        return {"similarity": sim, "rank": scores_loss_rank(sim.detach(), self._mode)[1]}

    def loss(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> Dict[str, torch.Tensor]:
        return {"softmax_cross_entropy": scores_loss_rank(predictions["similarity"], self._mode, self._weights(batch))[0]}

    def head(self, u: torch.Tensor, v: torch.Tensor, weights: Optional[torch.Tensor] = None):
        """the towers' embeddings -> ({"softmax_cross_entropy": loss}, {"rank": rank[, "similarity": sim]}) on the fused head"""
        loss, rank, sim = match_softmax(u, v, self._mode, self._cosine, self._temperature, weights, want_sim=self.want_similarity)
        predictions = {"rank": rank}
        if sim is not None:
            predictions["similarity"] = sim
        return {"softmax_cross_entropy": loss}, predictions

    def loss_and_predictions(self, batch: Batch):
        u, v = self._embeddings(batch)
        return self.head(u, v, self._weights(batch))
