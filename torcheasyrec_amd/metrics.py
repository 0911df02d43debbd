"""Evaluation from the config: `model_config.metrics` (and each task tower's) with the state on the device.

The reference's `train_and_evaluate` updates torchmetrics modules per eval step (`RankModel.update_metric`,
tzrec/models/rank_model.py:375-443) and computes them at the end (`compute_metric`): binned AUROC
(thresholds = 200), `tzrec/metrics/grouped_auc.py`, `tzrec/metrics/normalized_entropy.py`.  Here an update is one launch of
`csrc/eval_metrics.hip` per task tower (`tzr_metric_update`: histogram over (threshold bin, class) and the three NE sums) plus
one per grouped AUC (`tzr_grouped_auc_append`), with no host round trip -- the whole evaluation step (forward and every
update) replays from a hipGraph (`evaluate(..., graph=True)`).  `compute()` is where the host looks.

    ev = Evaluator(model, spec, device)
    print(evaluate(model, batches, ev))          # {"auc": ..., "grouped_auc": ..., "normalized_entropy": ...}
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import torch

from . import _lib
from .config import MetricSpec, PipelineSpec
from .embedding_group import BASE_DATA_GROUP, Batch, _batch_tensors, zch_wrapper_of

BUILT_KINDS = ("auc", "grouped_auc", "normalized_entropy", "recall_at_k")


def _world(pg) -> int:
    import torch.distributed as dist

    return dist.get_world_size(pg) if pg is not None and dist.is_available() and dist.is_initialized() else 1


def _all_reduce_sum(t: torch.Tensor, pg) -> torch.Tensor:
    import torch.distributed as dist

    from .sharding import stream_collective

    stream_collective(dist.all_reduce, t, op=dist.ReduceOp.SUM, group=pg)
    return t


def _inputs(probs: torch.Tensor, labels: torch.Tensor):
    """what the kernels read: float32 probabilities and int64 labels (as Batch carries them), dense, one per sample"""
    probs = probs.detach().reshape(-1).to(torch.float32).contiguous()
    labels = labels.detach().reshape(-1).to(torch.int64).contiguous()
    if probs.numel() != labels.numel():
        raise ValueError(f"metric update: {probs.numel()} predictions for {labels.numel()} labels")
    return probs, labels


def metric_update(probs: torch.Tensor, labels: torch.Tensor, auc: Optional["BinnedAUC"] = None,
                  ne: Optional["NormalizedEntropy"] = None) -> None:
    """One launch for the `auc` and the `normalized_entropy` of one tower (either may be None, not both)."""
    probs, labels = _inputs(probs, labels)
    p = _lib.ptr
    rc = _lib.lib().tzr_metric_update(
        p(probs), p(labels), probs.numel(), p(auc.thresholds) if auc is not None else None, auc.num_thresholds if auc is not None else 0,
        p(auc._hist) if auc is not None else None, p(ne._state) if ne is not None else None, _lib.stream_ptr(probs.device))
    _lib.check(rc, "tzr_metric_update")


class BinnedAUC:
    """`auc { thresholds: T }`: torchmetrics' binned binary AUROC.  State: int64[(T + 1), 2] counts of (bin, class), bin(p) =
    the number of thresholds <= p; the reference's [T, 2, 2] confusion matrix (decay_auc.py:31-35) is its suffix sums."""

    def __init__(self, thresholds: int = 200, device=None, process_group=None) -> None:
        T = int(thresholds)
        if T < 2:
            raise ValueError(f"auc: thresholds must be >= 2 (got {T})")
        if T > _lib.METRIC_MAX_THRESHOLDS:
            raise NotImplementedError(f"auc: {T} thresholds; the update kernel holds {_lib.METRIC_MAX_THRESHOLDS} per workgroup")
        self.num_thresholds, self._pg = T, process_group
        self.thresholds = torch.linspace(0, 1, T).to(device)  # (made on the host, as the reference's buffer is: the same floats)
        self._hist = torch.zeros((T + 1) * 2, dtype=torch.int64, device=device)

    def update(self, probs: torch.Tensor, labels: torch.Tensor) -> None:
        metric_update(probs, labels, auc=self)

    def reset(self) -> None:
        self._hist.zero_()

    def histogram(self) -> torch.Tensor:
        """int64 [T + 1, 2], summed over the ranks"""
        h = self._hist.clone()
        if _world(self._pg) > 1:
            _all_reduce_sum(h, self._pg)
        return h.view(-1, 2)

    def confmat(self) -> torch.Tensor:
        """int64 [T, 2, 2] indexed [threshold, target, prediction], prediction = (p >= threshold): [[tn, fp], [fn, tp]]"""
        h = self.histogram()
        total = h.sum(dim=0)
        ge = total[None, :] - torch.cumsum(h, dim=0)[:-1]  # [T, 2]: samples of each class in bins > t
        fp, tp = ge[:, 0], ge[:, 1]
        return torch.stack([torch.stack([total[0] - fp, fp], dim=1), torch.stack([total[1] - tp, tp], dim=1)], dim=1)

    def compute(self) -> torch.Tensor:
        c = self.confmat().to(torch.float64)
        tp, fp, fn, tn = c[:, 1, 1], c[:, 0, 1], c[:, 1, 0], c[:, 0, 0]
        zero = torch.zeros_like(tp)
        tpr = torch.where(tp + fn > 0, tp / (tp + fn), zero).flip(0)
        fpr = torch.where(fp + tn > 0, fp / (fp + tn), zero).flip(0)
        return torch.trapz(tpr, fpr)


class NormalizedEntropy:
    """`normalized_entropy { eta }` (tzrec/metrics/normalized_entropy.py).  State: float64 {sum ce, samples, sum labels}."""

    def __init__(self, eta: float = 1e-12, device=None, process_group=None) -> None:
        self.eta, self._pg = float(eta), process_group
        self._state = torch.zeros(3, dtype=torch.float64, device=device)

    def update(self, probs: torch.Tensor, labels: torch.Tensor) -> None:
        metric_update(probs, labels, ne=self)

    def reset(self) -> None:
        self._state.zero_()

    def state(self) -> torch.Tensor:
        s = self._state.clone()
        if _world(self._pg) > 1:
            _all_reduce_sum(s, self._pg)
        return s

    def compute(self) -> torch.Tensor:
        ce, n, pos = self.state().unbind()
        mean = (pos / n).clamp(self.eta, 1.0 - self.eta)
        norm = -(pos * torch.log(mean) + (n - pos) * torch.log(1.0 - mean))
        return (ce / norm).to(torch.float32)


class GroupedAUC:
    """`grouped_auc { grouping_key }` (tzrec/metrics/grouped_auc.py): the mean over the groups that hold both classes of the
    group's exact AUC.  Rows (prob, label, key) are appended to device buffers of `capacity` rows at a device-side cursor;
    `compute()` sorts them by (key, prob) and reduces.  Rows beyond the capacity are counted, not kept: `compute()` raises."""

    def __init__(self, capacity: int = 1 << 20, device=None, process_group=None) -> None:
        self.capacity, self._pg = int(capacity), process_group
        if self.capacity < 0:
            raise ValueError("grouped_auc: capacity < 0")
        self._probs = torch.zeros(self.capacity, dtype=torch.float32, device=device)
        self._labels = torch.zeros(self.capacity, dtype=torch.int32, device=device)
        self._keys = torch.zeros(self.capacity, dtype=torch.int64, device=device)
        self._state = torch.zeros(4, dtype=torch.int64, device=device)  # {cursor, overflow, arrivals, -}

    def update(self, probs: torch.Tensor, labels: torch.Tensor, grouping_key: torch.Tensor) -> None:
        probs, labels = _inputs(probs, labels)
        keys = grouping_key.detach().reshape(-1).to(torch.int64).contiguous()
        if keys.numel() != probs.numel():
            raise ValueError(f"grouped_auc update: {keys.numel()} keys for {probs.numel()} predictions")
        p = _lib.ptr
        rc = _lib.lib().tzr_grouped_auc_append(p(probs), p(labels), p(keys), probs.numel(), p(self._probs), p(self._labels), p(self._keys),
                                               self.capacity, p(self._state), _lib.stream_ptr(probs.device))
        _lib.check(rc, "tzr_grouped_auc_append")

    def reset(self) -> None:
        self._state.zero_()

    def rows(self):
        """(probs, labels, keys) held so far and the number of rows that did not fit"""
        n, overflow = self._state[:2].tolist()
        return self._probs[:n], self._labels[:n], self._keys[:n], int(overflow)

    @staticmethod
    def reduce_rows(probs: torch.Tensor, labels: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
        """float64 [2] = {sum of the per-group AUCs, groups counted} of these rows"""
        # two stable sorts: by prob, then by key -> (key, prob)
        probs, by_prob = torch.sort(probs, stable=True)
        keys, by_key = torch.sort(keys[by_prob], stable=True)
        probs, labels = probs[by_key].contiguous(), labels[by_prob][by_key].contiguous()
        n, dev = int(keys.numel()), keys.device
        L = _lib.lib()
        nbytes = L.tzr_grouped_auc_reduce_workspace(n)
        ws = _lib.workspace(nbytes, dev)
        auc_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        groups = torch.zeros(1, dtype=torch.int64, device=dev)
        p = _lib.ptr
        rc = L.tzr_grouped_auc_reduce(p(keys), p(probs), p(labels), n, p(auc_sum), p(groups), p(ws), nbytes, _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_grouped_auc_reduce")
        return torch.cat([auc_sum, groups.to(torch.float64)])

    def compute(self) -> torch.Tensor:
        probs, labels, keys, overflow = self.rows()
        world = _world(self._pg)
        if world > 1:
            over = _all_reduce_sum(torch.tensor([overflow], dtype=torch.int64, device=keys.device), self._pg)
            overflow = int(over.item())
        if overflow:
            raise RuntimeError(f"grouped_auc: {overflow} rows did not fit the capacity of {self.capacity} rows: build it larger")
        if world > 1:
            probs, labels, keys = self._exchange(probs, labels, keys, world)
        out = self.reduce_rows(probs, labels, keys)
        if world > 1:
            _all_reduce_sum(out, self._pg)
        return out[0] / out[1]

    def _exchange(self, probs, labels, keys, world: int):
        """every rank's rows to every rank; a rank keeps the groups with key % world == rank (the split the reference makes
        at update time, grouped_auc.py:44-90: the same groups meet on the same rank)"""
        import torch.distributed as dist

        from .sharding import stream_collective

        dev, n = keys.device, keys.numel()
        counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        stream_collective(lambda t, **kw: dist.all_gather(counts, t, **kw), torch.tensor([n], dtype=torch.int64, device=dev), group=self._pg)
        counts = [int(c.item()) for c in counts]
        width = max(counts + [1])
        out = []
        for t in (probs, labels, keys):
            padded = torch.zeros(width, dtype=t.dtype, device=dev)
            padded[:n] = t
            parts = [torch.zeros(width, dtype=t.dtype, device=dev) for _ in range(world)]
            stream_collective(lambda x, **kw: dist.all_gather(parts, x, **kw), padded, group=self._pg)
            out.append(torch.cat([q[:c] for q, c in zip(parts, counts)]))
        keep = out[2].remainder(world) == dist.get_rank(self._pg)
        return out[0][keep], out[1][keep], out[2][keep]


class RecallAtK:
    """`recall_at_k { top_k }` of a match model (tzrec/metrics/recall_at_k.py): the share of the samples whose positive is among
    the k highest scores of its row.  `update(rank)` takes the rank of the positive -- the number of other columns with a
    strictly higher score, what the similarity head counts while it walks the scores -- and adds sum_i [rank_i < k] and the number
    of rows to two int64 device counters: no host round trip, capturable.

    Without ties this equals the reference's `argsort(descending)[:, :k]` / `gather` of the one-hot label (recall_at_k.py:44-49).
    With ties the reference's result depends on the order its sort leaves equal scores in; here a tie never counts against the
    positive."""

    def __init__(self, top_k: int = 5, device=None, process_group=None) -> None:
        self.top_k, self._pg = int(top_k), process_group
        if self.top_k < 1:
            raise ValueError(f"recall_at_k: top_k must be >= 1 (got {top_k})")
        self._state = torch.zeros(2, dtype=torch.int64, device=device)  # {hits, rows}

    def update(self, rank: torch.Tensor) -> None:
        rank = rank.detach().reshape(-1)
        self._state[0] += (rank < self.top_k).sum()
        self._state[1] += rank.numel()

    def reset(self) -> None:
        self._state.zero_()

    def compute(self) -> torch.Tensor:
        s = self._state.clone()
        if _world(self._pg) > 1:
            _all_reduce_sum(s, self._pg)
        return (s[0].to(torch.float64) / s[1].to(torch.float64)).to(torch.float32)


def first_id_per_sample(kjt, key: str) -> torch.Tensor:
    """`kjt[key].to_padded_dense(1)[:, 0]` (rank_model.py:418-420): the first id of every sample, 0 for an empty bag --
    from the device tensors alone (`kjt[key]` asks the host for the key's extent), so it can be captured."""
    i, B = kjt.keys().index(key), kjt.stride()
    values = kjt.values()
    u = kjt.uniform_length()
    if u:
        return values.view(len(kjt.keys()), B, u)[i, :, 0]
    if values.numel() == 0:
        return torch.zeros(B, dtype=torch.int64, device=values.device)
    start = kjt.offsets()[i * B:(i + 1) * B]
    lengths = kjt.lengths()[i * B:(i + 1) * B]
    first = values[start.clamp(max=values.numel() - 1)]
    return torch.where(lengths > 0, first, torch.zeros_like(first))


class Evaluator:
    """One metric object per `MetricSpec` of the config, keyed by the reference's names: the kind plus `_<tower>` for a task
    tower's.  Kinds that are not built raise here, by name."""

    def __init__(self, model, spec: PipelineSpec, device=None, grouped_auc_capacity: int = 1 << 20) -> None:
        self._pg = getattr(model, "_pg", None)
        # a model with several towers per task (pepnet's domains): the per-sample choice among them, as its loss makes it
        self._select = getattr(model, "select_domain_predictions", None)
        self.device = torch.device(device) if device is not None else None
        self.metrics: Dict[str, object] = {}
        self._specs: Dict[str, MetricSpec] = {}
        self._recalls: List[str] = []  # the match models' metrics: fed predictions["rank"], no label
        # which predictions a model-level metric reads: "" unless the model says otherwise (`metric_suffixes()`; rocket_launching
        # in evaluation: "_light", keyed auc_light as the reference's update_metric does); a task tower's metric reads its tower's
        model_suffixes = list(model.metric_suffixes()) if hasattr(model, "metric_suffixes") else [""]
        self._suffix: Dict[str, str] = {}
        for ms, extra in [(ms, extra) for ms in spec.metrics for extra in ([""] if ms.tower else model_suffixes)]:
            if ms.kind == "recall_at_k":  # keyed recall@<k> (match_model.py:345-356)
                name = f"recall@{int(ms.fields.get('top_k', 5))}" + ms.suffix
                if name in self.metrics:
                    raise ValueError(f"metric {name!r} is configured twice")
                self.metrics[name] = RecallAtK(int(ms.fields.get("top_k", 5)), device=device, process_group=self._pg)
                self._recalls.append(name)
                continue
            if ms.kind == "auc":
                m = BinnedAUC(int(ms.fields.get("thresholds", 200)), device=device, process_group=self._pg)
            elif ms.kind == "normalized_entropy":
                m = NormalizedEntropy(float(ms.fields.get("eta", 1e-12)), device=device, process_group=self._pg)
            elif ms.kind == "grouped_auc":
                m = GroupedAUC(grouped_auc_capacity, device=device, process_group=self._pg)
            else:
                raise NotImplementedError(f"metric {ms.kind!r} is not built (built: {', '.join(BUILT_KINDS)})")
            name = ms.name + extra
            if name in self.metrics:
                raise ValueError(f"metric {name!r} is configured twice")
            self.metrics[name], self._specs[name], self._suffix[name] = m, ms, ms.suffix + extra
        # per tower: the `auc` and the `normalized_entropy` share a launch
        self._towers: Dict[str, List[str]] = {}
        for name in self._specs:
            self._towers.setdefault(self._suffix[name], []).append(name)
        # a two-class softmax output: `auc` / `grouped_auc` read the positive class's column (rank_model.py:392-416)
        self._probs_key: Dict[str, str] = {}
        for suffix in self._towers:
            t = spec.tower(suffix[1:]) if suffix and hasattr(spec, "tower") else None
            num_class = t.num_class if t is not None else int(getattr(spec, "num_class", 1))
            self._probs_key[suffix] = ("probs1" if num_class == 2 else "probs") + suffix

    def update(self, predictions: Dict[str, torch.Tensor], batch: Batch) -> None:
        if self._select is not None:
            predictions = self._select(predictions, batch)
        for name in self._recalls:
            self.metrics[name].update(predictions["rank"])
        for suffix, names in self._towers.items():
            probs = predictions[self._probs_key[suffix]]
            by_kind = {self._specs[n].kind: n for n in names}
            label = batch.labels[self._specs[names[0]].label]
            if "auc" in by_kind or "normalized_entropy" in by_kind:
                metric_update(probs, label, auc=self.metrics.get(by_kind.get("auc")), ne=self.metrics.get(by_kind.get("normalized_entropy")))
            if "grouped_auc" in by_kind:
                n = by_kind["grouped_auc"]
                key = first_id_per_sample(batch.sparse_features[BASE_DATA_GROUP], str(self._specs[n].fields["grouping_key"]))
                self.metrics[n].update(probs, label, key)

    def compute(self) -> Dict[str, torch.Tensor]:
        return {name: m.compute() for name, m in self.metrics.items()}

    def reset(self) -> None:
        for m in self.metrics.values():
            m.reset()


def _hints(b: Batch):
    """per sparse group: the one-id-per-bag hints of its KeyedJaggedTensor (of the one behind an int32 wire form)"""
    kjts = [(g, getattr(k, "_kjt", k)) for g, k in sorted(b.sparse_features.items())]
    return [(g, k.uniform_length(), k._uniform_keys) for g, k in kjts]


class _GraphEval:
    """forward + every metric update of one batch, captured once over a device batch with static addresses; later batches are
    copied into it in place (what GraphTrainPipeline._stage does for the training step) and the graph replayed."""

    def __init__(self, model, evaluator: Evaluator, device: torch.device) -> None:
        import torch.distributed as dist

        if device.type != "cuda":
            raise RuntimeError("evaluate(graph=True) replays a hipGraph: CUDA/HIP device only")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("evaluate(graph=True) captures the forward in one hipGraph: single-process models only")
        if zch_wrapper_of(model) is not None:
            raise NotImplementedError("evaluate(graph=True) of a model with a zero-collision hash")
        self._model, self._ev, self._device = model, evaluator, device
        self._slot: Optional[Batch] = None
        self._graph = None

    def _refresh(self, hb: Batch) -> None:
        if hb.sequence_mulval_lengths or hb.sequence_dense_features:
            raise ValueError("evaluate(graph=True) needs batches of dense, sparse and label tensors only")
        # the one-id-per-bag hints pick the lookups' kernels and which tensors are refreshed at all: a batch that differs in
        # them from the captured one would be read wrongly, silently
        if _hints(hb) != self._hints:
            raise ValueError("evaluate(graph=True): the batch's uniform-length hints differ from the captured batch's")
        src, dst = _batch_tensors(hb), _batch_tensors(self._slot)
        narrow = lambda a, b: a.dtype == torch.int32 and b.dtype == torch.int64  # noqa: E731 -- ids on the int32 wire
        if len(src) != len(dst) or any(a.shape != b.shape or (a.dtype != b.dtype and not narrow(a, b)) for a, b in zip(src, dst)):
            raise ValueError("evaluate(graph=True) needs fixed-shape batches (shapes changed between batches)")
        for a, b in zip(src, dst):
            b.copy_(a, non_blocking=True)

    def step(self, hb: Batch, eager: bool) -> None:
        if self._slot is None:
            self._slot, self._hints = hb.to(self._device), _hints(hb)
        else:
            self._refresh(hb)
        if eager:
            self._ev.update(self._model(self._slot), self._slot)
            return
        if self._graph is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._ev.update(self._model(self._slot), self._slot)
            self._graph = g
        self._graph.replay()


def evaluate(model, batches: Iterable[Batch], evaluator: Evaluator, graph: bool = False, warmup: int = 1) -> Dict[str, torch.Tensor]:
    """Forward only -- `model.eval()`, `torch.no_grad()`: no backward, so the fused sparse optimizer never runs and no
    parameter moves -- and the metric updates, over every batch; returns `evaluator.compute()`.  `graph=True`: the first
    `warmup` batches step eagerly (they load every kernel the step uses), then forward and updates are captured once
    and replayed per batch."""
    device = evaluator.device
    if device is None:
        device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    runner = _GraphEval(model, evaluator, device) if graph else None
    try:
        with torch.no_grad():
            for i, hb in enumerate(batches):
                if runner is not None:
                    runner.step(hb, eager=i < max(int(warmup), 1))
                else:
                    b = hb.to(device)
                    evaluator.update(model(b), b)
    finally:
        model.train(was_training)
    return evaluator.compute()
