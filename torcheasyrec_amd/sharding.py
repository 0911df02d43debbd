"""Sharded EmbeddingBagCollection: one process per GPU, RCCL over xGMI.

What it replaces.  In the reference, `DistributedModelParallel(module, plan, sharders)`
(/root/reference/tzrec/utils/dist_util.py:164-195, /root/reference/tzrec/main.py:783-804) swaps the
EBC for torchrec's sharded EBC [upstream 1.7.0]: KJTAllToAll (input dist) -> per-shard TBE lookup
-> PooledEmbeddingsReduceScatter / AllToAll (output dist), with the sharding type per table chosen
by the planner (`data_parallel | table_wise | row_wise | ...`,
/root/reference/tzrec/protos/feature.proto:6-13).

Placement ("plan", `make_plan`).
  * `row_wise`: contiguous blocks of ceil(rows/W) rows (torchrec geometry,
    /root/reference/tzrec/utils/plan_util.py:1049-1060); block q of table t lives on rank
    (q + rot[t]) mod W.  With block = rows this is table-wise placement on rank rot[t].
  * `data_parallel`: tables of at most `dp_max_rows` rows are replicated on every rank.  For
    DLRM-Criteo that is 18 of 26 tables = 7.75 MB of weights but 69 % of all lookups, which therefore
    never touch the network.

MI355X-first exchange.  xGMI is a point-to-point mesh, so bytes per link are what matters.
torchrec's row-wise output dist returns a dense [B_local, F*D] partial from every rank to every
rank (7/8 zeros when bags hold one id).  Here the row-wise exchange is at id granularity:

  forward   requester: K1 select the row-wise keys, K2 bucketize by owner -> all-to-all (ids)
            owner:     tzr_rows_gather, one embedding row per id          -> all-to-all (rows)
            requester: K5 pooled gather over the received rows (ids = unbucketize positions) and
                       K5 over the replicated tables, both straight into feature-group layout
  backward  requester: tzr_lookup_grads, one gradient row per id          -> all-to-all (rows)
            owner:     K6 plan + K7 fused optimizer with per-id gradients (grad_mode 1)
            replicas:  K6 + K7 in ACCUMULATE mode (exact per-row sums) -> ONE all-reduce of the
                       [sum rows, D] buffer -> tzr_dense_rows_update, identical on every rank

Dense parameters are data-parallel (gradients averaged like DDP, dist_util.py:170); sparse
gradients are summed over ranks, NOT divided by the world size (torchrec behaviour, SURVEY.md
appendix A.7).  One host sync per step sizes the all-to-all, as in torchrec.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import time

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from . import _lib
from .dlrm import MLP, OutputLinear
from .embedding import EmbeddingBagCollection, EmbeddingBagConfig, SparseOptimizerConfig
from .interaction import dot_interaction
from .sparse import KeyedJaggedTensor, block_bucketize
from .sparse_bwd import SparseBackward, direct_supported, grad_dsts


def row_wise_plan(rows: Sequence[int], world: int, whole: Optional[Sequence[bool]] = None) -> Tuple[List[int], List[int]]:
    """(block_size[t], rot[t]).  Tables with fewer blocks than ranks are rotated so their blocks
    land on different ranks (greedy by rows already placed).  `whole[t]` keeps table t in one
    block (table-wise placement: the rotation IS the owner rank)."""
    blocks = [max(1, r if (whole is not None and whole[i]) else -(-r // world)) for i, r in enumerate(rows)]
    load = [0] * world
    rot = []
    for r, b in zip(rows, blocks):
        nblk = -(-r // b)
        if nblk >= world:
            rot.append(0)
            for q in range(world):
                load[q] += min(b, max(0, r - q * b))
            continue
        best, best_cost = 0, None
        for o in range(world):
            cost = max(load[(q + o) % world] + min(b, r - q * b) for q in range(nblk))
            if best_cost is None or cost < best_cost:
                best, best_cost = o, cost
        rot.append(best)
        for q in range(nblk):
            load[(q + best) % world] += min(b, r - q * b)
    return blocks, rot


SHARDING_TYPES = ("data_parallel", "table_wise", "row_wise")


def _pg_of(group):
    return group if group is not None else dist.group.WORLD


def a2a_async(out: torch.Tensor, inp: torch.Tensor, group=None):
    """`dist.all_to_all_single(out, inp, async_op=True)` with equal splits, issued straight on the ProcessGroup object: the
    functional wrapper's argument checks and logging decorator were 10 - 15 us of host time per collective, five of them
    per sharded step (profiles/r04r)."""
    opts = dist.AllToAllOptions()
    opts.asyncOp = True
    return _pg_of(group).alltoall_base(out, inp, [], [], opts)


def allreduce_async(t: torch.Tensor, group=None, avg: bool = False):
    opts = dist.AllreduceOptions()
    opts.reduceOp = dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM
    opts.asyncOp = True
    return _pg_of(group).allreduce([t], opts)


def stream_collective(fn, tensor: torch.Tensor, *args, **kw):
    """A collective the caller needs complete IN STREAM ORDER (what `async_op=False` means), issued so that it is safe
    next to hipGraph captures.  torch's process group runs a sync collective ON the current stream and records its
    completion event there; its watchdog thread polls that event (hipEventQuery) until it has seen it complete, and on
    this ROCm stack a query of an event whose stream is CAPTURING fails (hipErrorCapturedEvent) -- the watchdog throws,
    the process aborts, and the capture is invalidated (round 3's intermittent abort; reproduced at will by
    scripts/capture_stress.py in round 4).  Issued async the collective runs on RCCL's own stream -- which nothing ever
    captures -- and `.wait()` makes the current stream wait for it: same ordering, no event of ours on a capturable
    stream.  CPU tensors (gloo): the plain blocking call."""
    if tensor.is_cuda:
        w = fn(tensor, *args, async_op=True, **kw)
        if w is not None:
            w.wait()
        return None
    return fn(tensor, *args, **kw)


def make_plan(tables: Sequence[EmbeddingBagConfig], world: int, dp_max_rows: int = 65536,
              replicate_at_world1: bool = False, constraints: Optional[Dict[str, str]] = None,
              tw_max_rows: int = 0) -> Dict[str, dict]:
    """{table: {"sharding_type": "data_parallel" | "table_wise" | "row_wise", "block", "rot",
    "ranks"}} -- the fields tzrec persists from torchrec's plan
    (tzrec/utils/checkpoint_util.py:1152-1167).

    `constraints[table]` pins a sharding type, with the meaning of tzrec's per-feature
    `embedding_constraints.sharding_types` (/root/reference/tzrec/features/feature.py:359-371).
    Unconstrained tables: <= dp_max_rows rows -> data_parallel, <= tw_max_rows -> table_wise, else
    row_wise.  (table_wise is opt-in: with one id per bag a whole table on one rank means that rank
    serves B lookups while its peers serve B/W, so row_wise balances better.)"""
    plan: Dict[str, dict] = {}
    constraints = constraints or {}
    for name, kind in constraints.items():
        if kind not in SHARDING_TYPES:
            raise ValueError(f"{name}: sharding type {kind!r} not supported (one of {SHARDING_TYPES})")
    # at world 1 replication is pointless (kept only as a switch to exercise that path on one GPU)
    small_ok = world > 1 or replicate_at_world1

    def kind_of(t):
        if t.name in constraints:
            return constraints[t.name]
        if small_ok and t.num_embeddings <= dp_max_rows:
            return "data_parallel"
        return "table_wise" if t.num_embeddings <= tw_max_rows else "row_wise"

    kinds = {t.name: kind_of(t) for t in tables}
    ex = [t for t in tables if kinds[t.name] != "data_parallel"]  # tables that take part in the exchange
    blocks, rot = row_wise_plan([t.num_embeddings for t in ex], world, [kinds[t.name] == "table_wise" for t in ex])
    placed = {t.name: (b, o) for t, b, o in zip(ex, blocks, rot)}
    for t in tables:
        if t.name in placed:
            b, o = placed[t.name]
            ranks = [o] if kinds[t.name] == "table_wise" else list(range(world))
            plan[t.name] = {"sharding_type": kinds[t.name], "block": b, "rot": o, "ranks": ranks}
        else:
            plan[t.name] = {"sharding_type": "data_parallel", "ranks": list(range(world))}
    return plan


class _ShardedLookupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, kjt, dst_names, hook):
        outs, state = mod._forward_impl(kjt, dst_names)
        ctx.mod, ctx.state = mod, state
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        ctx.mod._backward_impl(ctx.state, grads)
        return None, None, None, None


class ShardedEmbeddingBagCollection(nn.Module):
    """Sharded pooled lookup with the optimizer fused in backward.

    Same constructor surface as `EmbeddingBagCollection` (tables are the GLOBAL configs); all tables
    must share one embedding_dim (DLRM / the fm+deep groups of DeepFM) and every KJT key must feed
    exactly one table."""

    def __init__(
        self,
        tables: Sequence[EmbeddingBagConfig],
        device: torch.device,
        optimizer: Optional[SparseOptimizerConfig] = None,
        groups: Optional[Dict[str, List[str]]] = None,
        row_layout: str = "interleaved",
        process_group: Optional[dist.ProcessGroup] = None,
        dp_max_rows: int = 65536,
        replicate_at_world1: bool = False,
        constraints: Optional[Dict[str, str]] = None,
        tw_max_rows: int = 0,
        plan: Optional[Dict[str, dict]] = None,
        out_keys: Optional[Dict[Tuple[str, str], str]] = None,
        out_dims: Optional[Dict[str, int]] = None,
        exchange: str = "exact",
        capacity_factor: float = 1.25,
    ) -> None:
        """`exchange`: "exact" = split sizes through the host every step (counts all-to-all, D2H, sync);
        "capacity" = fixed slices of `capacity_factor` x the even share per destination, no read-back on the way
        (`input_dist_begin`), a batch that does not fit is redone through the exact exchange before anything
        uses it.  `out_keys[(feature, table)]`: name of that lookup's pooled block in `groups` (default: the
        feature name); `out_dims[block]`: width of blocks of `groups` that OTHER collections fill in the
        same output buffers (`MixedShardedEmbeddingBagCollection`: one collection per embedding dim)."""
        super().__init__()
        self.pg = process_group
        self.W = dist.get_world_size(self.pg)
        self.rank = dist.get_rank(self.pg)
        self._device = torch.device(device)
        self._global = list(tables)
        dims = {t.embedding_dim for t in tables}
        if len(dims) != 1:
            raise ValueError("sharded lookup needs one embedding_dim for all tables")
        self.dim = dims.pop()
        self._opt_cfg = optimizer
        # `plan`: the output of planner.plan_tables (or a plan restored from a checkpoint); otherwise
        # the size heuristic of make_plan
        self._plan = plan if plan is not None else make_plan(self._global, self.W, dp_max_rows, replicate_at_world1,
                                                             constraints, tw_max_rows)
        missing = [t.name for t in self._global if t.name not in self._plan]
        if missing:
            raise ValueError(f"sharding plan has no entry for {missing}")
        # table_wise is the one-block case of the row-wise exchange (block = rows, owner = rot)
        self._rw = [t for t in self._global if self._plan[t.name]["sharding_type"] != "data_parallel"]
        self._dp = [t for t in self._global if self._plan[t.name]["sharding_type"] == "data_parallel"]
        self.block = {t.name: self._plan[t.name]["block"] for t in self._rw}
        self.rot = {t.name: self._plan[t.name]["rot"] for t in self._rw}

        # --- row-wise shards owned by this rank ---
        local_cfgs = []
        for cfg in self._rw:
            lo, n = self.shard_of(cfg.name)
            if cfg.init_fn is not None:  # init the global table deterministically, keep my block
                def init(w, cfg=cfg, lo=lo, n=n):  # noqa: E306
                    full = torch.empty(cfg.num_embeddings, cfg.embedding_dim)
                    cfg.init_fn(full)
                    if n > 0:
                        w[:n].copy_(full[lo:lo + n])
            else:
                def init(w, rows=cfg.num_embeddings):  # noqa: E306
                    a = (1.0 / max(rows, 1)) ** 0.5  # same distribution as the unsharded table
                    w.uniform_(-a, a)
            local_cfgs.append(EmbeddingBagConfig(cfg.name, cfg.embedding_dim, max(n, 1), list(cfg.feature_names),
                                                 cfg.pooling, init, trainable=cfg.trainable, data_type=cfg.data_type))
        self.local = EmbeddingBagCollection(local_cfgs, device=self._device, optimizer=optimizer,
                                            row_layout=row_layout) if local_cfgs else None
        # --- replicated tables ---
        self.replica = EmbeddingBagCollection(
            [EmbeddingBagConfig(c.name, c.embedding_dim, c.num_embeddings, list(c.feature_names), c.pooling, c.init_fn,
                                trainable=c.trainable, data_type=c.data_type) for c in self._dp], device=self._device, optimizer=optimizer,
            row_layout=row_layout) if self._dp else None
        if self.replica is not None:
            for store in self.replica._storage:  # identical replicas: rank 0's values (and zero state)
                stream_collective(dist.broadcast, store, src=0, group=self.pg)
            for st in self.replica._states.values():
                if st.data_ptr() not in {s.data_ptr() for s in self.replica._storage}:
                    stream_collective(dist.broadcast, st, src=0, group=self.pg) if st.is_contiguous() else None
            rows = [c.num_embeddings for c in self._dp]
            self._dp_row_start = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int64, device=self._device)
            self._dp_rows = int(sum(rows))
            self._dp_acc = torch.zeros(self._dp_rows, self.dim, dtype=torch.float32, device=self._device)
        self.fused_optimizer = (self.local or self.replica).fused_optimizer
        if self.local is not None and self.replica is not None:  # one lr handle drives both
            self.replica.fused_optimizer.param_groups = self.local.fused_optimizer.param_groups
        # lookups in table-then-feature order of the GLOBAL config list
        self._lookups: List[Tuple[str, int, str]] = []  # (key, global table idx, out_key)
        for t, cfg in enumerate(self._global):
            for f in cfg.feature_names:
                self._lookups.append((f, t, (out_keys or {}).get((f, cfg.name), f)))
        self._out_dims = dict(out_dims or {})
        keys = [k for k, _, _ in self._lookups]
        if len(set(keys)) != len(keys):
            raise ValueError("a KJT key feeds more than one sharded table")
        self._groups = groups
        self._hook = torch.zeros(0, requires_grad=True, device=self._device)
        self._req_meta: Dict[Tuple, dict] = {}
        self._own_meta: Dict[bool, dict] = {}
        if exchange not in ("exact", "capacity"):
            raise ValueError(f"exchange = {exchange!r}: 'exact' or 'capacity'")
        self.exchange = exchange
        self.capacity_factor = float(capacity_factor)
        self.capacity_slack = 64  # ids on top of factor x even share (small batches are lumpy)
        # ragged / weighted bags: slices must have the SAME size on every rank, so they cannot follow a rank's own id
        # count -- they are sized for this many ids per bag on average (None: such batches take the exact exchange)
        self.capacity_bag_len: Optional[float] = None
        self.exchange_stats = {"capacity_batches": 0, "overflow_retries": 0}
        self.flag_wait_s = 0.0  # host time spent waiting for a batch's overflow word (the host ahead of the device, not busy)
        self.input_dist_group = None  # process group of the ids all-to-all (default: `process_group`); a step captured
        #                               in a hipGraph replays its collectives while the next batch's input dist runs
        self._slot_bufs: Dict[Tuple, dict] = {}
        self._rows_buf: Dict[int, tuple] = {}
        self._timers = None
        # set by ShardedManagedCollisionEmbeddingBagCollection: tables whose raw ids are routed by hash
        # and mapped to rows by their owner (`_owner_remap(st) -> row ids of the received lookups`)
        self._hash_routed = set()
        self._owner_remap = None
        self._lookup_trackers: list = []  # register_post_lookup_tracker_fn

    def register_post_lookup_tracker_fn(self, fn) -> None:
        """See EmbeddingBagCollection.register_post_lookup_tracker_fn.  A sharded collection reports what
        torchrec's post-lookup tracker sees: the LOCAL rows each rank serves as an owner (the ids
        received in the exchange, after the owner's zch remap) and its own lookups of replicated tables."""
        self._lookup_trackers.append(fn)

    # -- placement -------------------------------------------------------------------------------
    def shard_of(self, name: str) -> Tuple[int, int]:
        """(first global row, rows) of table `name` held by this rank (replicas: the whole table)."""
        cfg = next(c for c in self._global if c.name == name)
        if self._plan[name]["sharding_type"] == "data_parallel":
            return 0, cfg.num_embeddings
        b = self._plan[name]["block"]
        q = (self.rank - self._plan[name]["rot"]) % self.W
        lo = q * b
        return lo, max(0, min(b, cfg.num_embeddings - lo))

    def plan(self) -> Dict[str, dict]:
        return self._plan

    def table_weights(self) -> Dict[str, torch.Tensor]:
        out = {}
        for m in (self.local, self.replica):
            if m is not None:
                out.update(m.table_weights())
        return out

    def table_states(self) -> Dict[str, torch.Tensor]:
        out = {}
        for m in (self.local, self.replica):
            if m is not None:
                out.update(m.table_states())
        return out

    # -- descriptors ---------------------------------------------------------------------------
    def _layout_for(self, dst_names):
        if dst_names == ("__all__",):
            return [("__all__", [ok for _, _, ok in self._lookups])]
        return [(g, self._groups[g]) for g in dst_names]

    def _requester_meta(self, kjt_keys, layout) -> dict:
        ck = (tuple(kjt_keys), tuple((n, tuple(ks)) for n, ks in layout))
        m = self._req_meta.get(ck)
        if m is not None:
            return m
        key_index = {k: i for i, k in enumerate(kjt_keys)}
        # global column of every out_key in every destination
        where: Dict[str, List[Tuple[int, int]]] = {}
        for d, (_, out_keys) in enumerate(layout):
            col = 0
            for ok in out_keys:
                where.setdefault(ok, []).append((d, col))
                col += self._out_dims.get(ok, self.dim)
        pool = {c.name: c.pooling for c in self._global}
        rw_names = [c.name for c in self._rw]
        dp_names = [c.name for c in self._dp]

        def build(part_lookups, table_index, key_of):
            feats = np.zeros(len(part_lookups), dtype=_lib.FEATURE_DT)
            feats["dst"] = -1
            slots = []
            for i, (key, t, ok) in enumerate(part_lookups):
                feats[i]["table"] = table_index(t)
                feats[i]["key"] = key_of(key)
                feats[i]["pooling"] = _lib.POOL_MEAN if pool[self._global[t].name].lower() == "mean" else _lib.POOL_SUM
                feats[i]["order"] = i
                for n, (d, col) in enumerate(where.get(ok, [])):
                    feats[i]["dst"][n], feats[i]["col"][n] = d, col
                    feats[i]["n_dst"] = n + 1
                    for c in range(self.dim // 4):
                        slots.append((i, c, d, col + 4 * c))
            slots = np.array(slots, dtype=_lib.SLOT_DT)
            return feats, slots

        rw_lk = [lk for lk in self._lookups if self._global[lk[1]].name in self.block]
        dp_lk = [lk for lk in self._lookups if self._global[lk[1]].name not in self.block]
        for key, _, _ in self._lookups:
            if key not in key_index:
                raise KeyError(f"KeyedJaggedTensor has no key {key!r}")
        m = {"widths": [sum(self._out_dims.get(k, self.dim) for k in ks) for _, ks in layout]}
        if rw_lk:
            rw_keys = [k for k, _, _ in rw_lk]  # order of the permuted sub-KJT
            sub_index = {k: i for i, k in enumerate(rw_keys)}
            feats, slots = build(rw_lk, lambda t: 0, lambda k: sub_index[k])
            m.update({
                "rw_perm": [key_index[k] for k in rw_keys], "rw_feats_np": feats, "rw_slots_n": len(slots),
                "rw_sel": torch.tensor([key_index[k] for k in rw_keys], dtype=torch.int32, device=self._device),
                "rw_d_feats": _lib.upload_struct(feats, self._device), "rw_d_slots": _lib.upload_struct(slots, self._device),
                # block 0 = hash routing of raw ids (zero-collision-hash tables, see zch.py)
                "rw_blk": torch.tensor([0 if self._global[t].name in self._hash_routed else self.block[self._global[t].name]
                                        for _, t, _ in rw_lk], dtype=torch.int64, device=self._device),
                "rw_rot": torch.tensor([self.rot[self._global[t].name] for _, t, _ in rw_lk], dtype=torch.int32, device=self._device),
                "rw_key_table": np.array([rw_names.index(self._global[t].name) for _, t, _ in rw_lk], dtype=np.int32),
                "rw_n": len(rw_lk),
            })
        if dp_lk:
            feats, slots = build(dp_lk, lambda t: dp_names.index(self._global[t].name), lambda k: key_index[k])
            # table descriptors of the replicas (weights + real state) and their ACCUMULATE twin
            base = self.replica._meta([lk.key for lk in self.replica._lookups], self.replica._default_layout())
            tables = base.tables_np.copy()
            acc_tables = tables.copy()
            rs = self._dp_row_start.cpu().numpy()
            for t in range(len(tables)):
                mine = [i for i, (_, tt, _) in enumerate(dp_lk) if dp_names.index(self._global[tt].name) == t]
                for arr in (tables, acc_tables):
                    arr[t]["first_order"] = mine[0] if mine else 0
                    arr[t]["n_feats"] = len(mine)
                acc_tables[t]["m"] = self._dp_acc.data_ptr() + int(rs[t]) * self.dim * 4
                acc_tables[t]["m_stride"] = self.dim
            # backward twins: lookups of frozen replicas accumulate nothing (their rows of the accumulation
            # buffer stay zero, and a zero row gradient is a row the dense update skips)
            frozen = [not c.trainable for c in self._dp]
            bwd_feats = feats
            if any(frozen):
                from .embedding import mask_frozen_descriptors

                acc_tables, bwd_feats = mask_frozen_descriptors(acc_tables, feats, frozen)
            m.update({
                "dp_feats_np": feats, "dp_slots_n": len(slots), "dp_n": len(dp_lk),
                "dp_d_feats": _lib.upload_struct(feats, self._device), "dp_d_slots": _lib.upload_struct(slots, self._device),
                "dp_d_bwd_feats": _lib.upload_struct(bwd_feats, self._device),
                "dp_d_tables": _lib.upload_struct(tables, self._device),
                "dp_d_acc_tables": _lib.upload_struct(acc_tables, self._device),
                "dp_max_rows": int(max(c.num_embeddings for c in self._dp)), "n_keys": len(kjt_keys),
            })
        self._req_meta[ck] = m
        return m

    def _owner_meta(self, key_table: np.ndarray, capped: bool = False) -> dict:
        """Descriptors of the owner side: W*F received keys (source-major), key (s, f) -> table.
        `capped`: the key list of the capacity-bounded message (`tzr_exchange_owner_segments`): per source
        rank one dead key (table -1) ahead of its F keys, one more dead key at the end."""
        hit = self._own_meta.get(capped)
        if hit is not None:
            return hit
        F, W, T = len(key_table), self.W, len(self._rw)
        if capped:
            kt = np.concatenate([np.concatenate([[-1], key_table]) for _ in range(W)] + [[-1]]).astype(np.int32)
        else:
            kt = np.tile(key_table, W).astype(np.int32)
        K = len(kt)
        real = np.nonzero(kt >= 0)[0]
        base = self.local._meta([lk.key for lk in self.local._lookups], self.local._default_layout())
        tables = base.tables_np.copy()
        feats = np.zeros(K, dtype=_lib.FEATURE_DT)
        feats["dst"] = -1
        order = np.lexsort((np.arange(K), np.where(kt >= 0, kt, T)))  # table-major order of the received keys, dead last
        rank_of = np.empty(K, dtype=np.int32)
        rank_of[order] = np.arange(K, dtype=np.int32)
        feats["table"], feats["key"], feats["order"] = kt, np.arange(K, dtype=np.int32), rank_of
        for t in range(T):
            mine = np.nonzero(kt == t)[0]
            tables[t]["first_order"] = int(rank_of[mine].min()) if len(mine) else 0
            tables[t]["n_feats"] = len(mine)
        frozen = [not c.trainable for c in self.local.embedding_bag_configs()]
        bwd_tables, bwd_feats = tables, feats
        if any(frozen) or capped:
            from .embedding import mask_frozen_descriptors

            bwd_tables, bwd_feats = mask_frozen_descriptors(tables, feats, frozen)
        names = [c.name for c in self._rw]
        hit = {
            "d_tables": _lib.upload_struct(tables, self._device),
            "d_feats": _lib.upload_struct(feats, self._device),
            "d_bwd_tables": _lib.upload_struct(bwd_tables, self._device),
            "d_bwd_feats": _lib.upload_struct(bwd_feats, self._device),
            "d_key_table": torch.from_numpy(kt).to(self._device), "K": K, "T": T,
            "max_rows": int(max(c.num_embeddings for c in self.local.embedding_bag_configs())),
            "track_segs": tuple((names[int(kt[k])], int(k)) for k in real),
        }
        self._own_meta[capped] = hit
        return hit

    def _recv_rows_buffer(self, n: int, n_lookups: int):
        """Persistent [n, D] buffer for the rows coming back from their owners plus the one-table
        descriptor that lets K5 pool over it (cached: no per-step upload)."""
        hit = self._rows_buf.get(n)
        if hit is None:
            D = self.dim
            rows_in = torch.empty(max(n, 1), D, dtype=torch.float32, device=self._device)
            pt = np.zeros(1, dtype=_lib.TABLE_DT)
            pt[0]["w"], pt[0]["rows"], pt[0]["dim"], pt[0]["w_stride"] = rows_in.data_ptr(), max(n, 1), D, D
            pt[0]["n_feats"] = n_lookups
            hit = (rows_in, _lib.upload_struct(pt, self._device))
            if len(self._rows_buf) > 8:
                self._rows_buf.clear()
            self._rows_buf[n] = hit
        return hit

    # -- exchange ------------------------------------------------------------------------------
    def _a2a(self, out: torch.Tensor, inp: torch.Tensor, out_splits, in_splits, async_op: bool = False):
        """async_op=True: the collective runs on RCCL's stream while the caller keeps queueing local
        kernels; `.wait()` makes the current stream wait for it (no host block on a GPU)."""
        if async_op:
            return dist.all_to_all_single(out, inp, out_splits, in_splits, group=self.pg, async_op=True)
        return stream_collective(dist.all_to_all_single, out, inp, out_splits, in_splits, group=self.pg)

    def _optim_struct(self, kind: Optional[int] = None):
        return self.fused_optimizer.optim_struct(self._device, kind)

    # The forward is three host-visible pieces so a train pipeline can run the first two one batch
    # ahead on a side stream (the reference's TrainPipelineSparseDist does the same with torchrec's
    # input_dist, /root/reference/tzrec/utils/dist_util.py:221-303):
    #   input_dist_begin  bucketize by owner, exchange the per-(rank, key) counts, start their D2H copy
    #   input_dist_end    wait for the counts (the one host sync of a step), ids all-to-all
    #   lookup            owner row gather, rows all-to-all, pooled gather into the output buffers
    def exchange_capacity(self, n_keys: int, B: int, n_ids: Optional[int] = None) -> int:
        """ids one rank may send to one destination per batch in the capacity-bounded exchange (`n_ids`: the
        batch's id count when bags are ragged; default one id per bag)"""
        if n_ids is None:
            total = n_keys * B
            return max(1, min(total, int(np.ceil(self.capacity_factor * total / self.W)) + self.capacity_slack))
        # ragged bags: sized from the configured average bag length, NOT from n_ids (which differs between ranks)
        return max(1, int(np.ceil(self.capacity_factor * n_keys * B * float(self.capacity_bag_len) / self.W)) + self.capacity_slack)

    def _slot(self, slot, what: str, shape, dtype, pinned: bool = False) -> torch.Tensor:
        """Persistent buffer `what` of pipeline slot `slot` (None: a fresh tensor).  A captured step reads the
        input dist's products at fixed addresses; two slots alternate so batch i+1 is laid out while i runs."""
        if slot is None:
            return torch.empty(shape, dtype=dtype, pin_memory=True) if pinned else torch.empty(shape, dtype=dtype, device=self._device)
        key = (slot, what, tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),), dtype)
        hit = self._slot_bufs.get(key)
        if hit is None:
            hit = torch.empty(shape, dtype=dtype, pin_memory=True) if pinned else torch.empty(shape, dtype=dtype, device=self._device)
            self._slot_bufs[key] = hit
        return hit

    def _slot_workspace(self, slot, what: str, nbytes: int) -> torch.Tensor:
        if slot is None:
            return _lib.workspace(nbytes, self._device)
        t = self._slot(slot, what, int(nbytes) + 256, torch.uint8)
        return t[(-t.data_ptr()) % 256:]

    # the capacity-bounded input dist in its pieces (a pipeline replays the kernel runs from hipGraphs: with a slot
    # every buffer below is persistent, so `cap_state` is host work only)
    def cap_state(self, st: dict, slot, n_ids: Optional[int] = None) -> dict:
        kjt, rm, W = st["kjt"], st["rm"], self.W
        B, F = kjt.stride(), rm["rw_n"]
        N = F * B if n_ids is None else int(n_ids)
        C = self.exchange_capacity(F, B, n_ids)
        S = int(_lib.lib().tzr_exchange_message_stride(F, C))
        msg = self._slot(slot, "msg", (2, W * S), torch.int64)  # [0] what I send, [1] what I receive
        seg = self._slot(slot, "seg", W * (F + 1) + 3, torch.int64)  # key starts, then the overflow word
        host = self._slot(slot, "flag", 1, torch.int64, pinned=True) if self._device.type == "cuda" else seg[-1:]
        st.update({"cap": C, "sub": None, "N_rw": N, "N_pad": W * S, "unb": self._slot(slot, "unb", N, torch.int64), "msg": msg,
                   "recv_ids": msg[1], "seg": seg, "key_start": seg[:-1], "n_recv": W * S, "send_splits": None,
                   "recv_splits": None, "om": self._owner_meta(rm["rw_key_table"], capped=True), "flag_host": host})
        return st

    def cap_bucketize(self, st: dict) -> None:
        L, dev, kjt, rm = _lib.lib(), self._device, st["kjt"], st["rm"]
        B, F = kjt.stride(), rm["rw_n"]
        ws = _lib.workspace(L.tzr_exchange_bucketize_workspace(F, B, self.W), dev)
        _lib.check(L.tzr_exchange_bucketize_capped(_lib.ptr(rm["rw_sel"]), F, _lib.ptr(rm["rw_blk"]), _lib.ptr(rm["rw_rot"]), B, 1, self.W,
                                                   _lib.ptr(kjt.values()), st["cap"], _lib.ptr(st["msg"][0]), _lib.ptr(st["unb"]),
                                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "tzr_exchange_bucketize_capped")

    def cap_exchange(self, st: dict) -> None:
        if st["msg"].is_cuda:
            a2a_async(st["msg"][1], st["msg"][0], self.input_dist_group or self.pg).wait()
        else:
            dist.all_to_all_single(st["msg"][1], st["msg"][0], group=self.input_dist_group or self.pg)

    def cap_segments(self, st: dict) -> None:
        seg = st["seg"]
        _lib.check(_lib.lib().tzr_exchange_owner_segments(_lib.ptr(st["msg"][1]), self.W, st["rm"]["rw_n"], st["cap"], _lib.ptr(seg),
                                                          _lib.ptr(seg[-1:]), _lib.stream_ptr(self._device)),
                   "tzr_exchange_owner_segments")
        if self._device.type == "cuda":
            self.cap_flag_arm(st)
            st["flag_host"].copy_(seg[-1:], non_blocking=True)

    def cap_flag_arm(self, st: dict) -> None:
        """Host side of the overflow word's trip: a sentinel in the pinned word BEFORE the D2H copy that will overwrite it is
        queued (or replayed from a graph: call this in front of the replay).  `input_dist_end` then polls the word itself --
        no event: hipEventSynchronize / hipEventQuery answered 60 - 150 us after the copy had landed (the event behind a
        hipGraph launch completes when the runtime's handler thread gets to it), the largest single item of a sharded
        step's host time (profiles/r04r, r04s)."""
        if self._device.type == "cuda":
            st["flag_host"].fill_(-1)
            st["flag_armed"] = True

    def cap_flag_event(self, st: dict) -> None:
        if self._device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self._device))
            st["flag_event"] = ev

    def cap_eligible(self, kjt: KeyedJaggedTensor, dst_names) -> bool:
        """would `input_dist_begin` take the capacity-bounded exchange for this batch?"""
        rm = self._requester_meta(kjt.keys(), self._layout_for(dst_names))
        return ("rw_n" in rm and self.exchange == "capacity" and kjt.uniform_length() == 1 and kjt.weights_or_none() is None
                and self.W <= 64 and self.W * rm["rw_n"] <= 256 and self._owner_remap is None and kjt.stride() > 0)

    def input_dist_begin(self, kjt: KeyedJaggedTensor, dst_names, exact: bool = False, slot=None) -> dict:
        dev, W = self._device, self.W
        layout = self._layout_for(dst_names)
        rm = self._requester_meta(kjt.keys(), layout)
        st = {"kjt": kjt, "rm": rm, "uniform": kjt.uniform_length() == 1, "dst_names": dst_names, "slot": slot}
        lean = "rw_n" in rm and st["uniform"] and kjt.weights_or_none() is None and W <= 64 and W * rm["rw_n"] <= 256
        if lean and self.exchange == "capacity" and not exact and self._owner_remap is None and kjt.stride() > 0:
            # fixed slices: ONE all-to-all carries counts, overflow word and ids; nothing is read back here
            self.cap_state(st, slot)
            self.cap_bucketize(st)
            self.cap_exchange(st)
            self.cap_segments(st)
            self.cap_flag_event(st)
            return st
        if "rw_n" in rm:
            B = kjt.stride()
            F = rm["rw_n"]
            cnt = torch.empty(2, W * F, dtype=torch.int64, device=dev)  # [0] ids I send per (dest, key); [1] ids I receive
            if lean:
                # one id per bag, no weights: the lean 3-launch bucketize on the selected keys (no K1
                # permute, no W*F*B bag lengths); same outputs as the general path below
                L = _lib.lib()
                sub = None
                N = F * B
                out_ids = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
                unb = torch.empty(max(N, 1), dtype=torch.int64, device=dev)
                ws = _lib.workspace(L.tzr_exchange_bucketize_workspace(F, B, W), dev)
                _lib.check(L.tzr_exchange_bucketize(_lib.ptr(rm["rw_sel"]), F, _lib.ptr(rm["rw_blk"]), _lib.ptr(rm["rw_rot"]), B, 1, W,
                                                    _lib.ptr(kjt.values()), _lib.ptr(out_ids), _lib.ptr(unb), _lib.ptr(cnt[0]),
                                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), "tzr_exchange_bucketize")
                bkt_values, unb = out_ids[:N], unb[:N]
            else:
                sub = kjt if rm["rw_perm"] == list(range(len(kjt.keys()))) else kjt.permute(rm["rw_perm"])
                N = sub.values().numel()
                bkt, unb = block_bucketize(sub, rm["rw_blk"], W, return_permute=True, rank_offsets=rm["rw_rot"])
                torch.sub(bkt.offsets()[B::B], bkt.offsets()[:-1:B], out=cnt[0])
                bkt_values = bkt.values()
                if (self.exchange == "capacity" and self.capacity_bag_len is not None and not exact and self._owner_remap is None
                        and W <= 64 and B > 0):
                    # ragged / weighted bags: the dense bucketize result re-laid into the fixed slices (tzr_exchange_pad)
                    self.cap_state(st, slot, n_ids=N)
                    st["sub"] = sub
                    _lib.check(_lib.lib().tzr_exchange_pad(_lib.ptr(cnt[0]), W, F, st["cap"], _lib.ptr(bkt_values), _lib.ptr(unb), N,
                                                           _lib.ptr(st["msg"][0]), _lib.ptr(st["unb"]), _lib.stream_ptr(dev)),
                               "tzr_exchange_pad")
                    self.cap_exchange(st)
                    self.cap_segments(st)
                    self.cap_flag_event(st)
                    return st
            self._a2a(cnt[1], cnt[0], None, None)
            recv_cnt = cnt[1]
            if dev.type == "cuda":  # per-rank totals are summed on the host: no extra launches
                host = torch.empty(cnt.shape, dtype=cnt.dtype, pin_memory=True)
                host.copy_(cnt, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                st["counts_event"] = ev
            else:
                host = cnt
            st.update({"sub": sub, "N_rw": N, "bkt_values": bkt_values, "unb": unb, "recv_cnt": recv_cnt, "counts_host": host})
        return st

    def input_dist_end(self, st: dict) -> dict:
        rm, dev, W = st["rm"], self._device, self.W
        if "cap" in st and "flag_host" in st:
            # the overflow word is the same on every rank (each slice carries its sender's, the owner kernel ORs
            # all W of them), so all ranks redo the batch together.  This IS a host wait: ShardedTrainStep calls
            # _end(_begin(next)) back to back, so the host blocks until the side stream has run the next batch's
            # bucketize + ids all-to-all + flag copy.  Those were queued behind the START of the current step only
            # and run beside it, while the host has already queued the whole current step: the wait ends long
            # before the main stream drains -- but it is a wait, not "recorded a batch ago" (ADVICE round 2).
            ev = st.pop("flag_event", None)
            if st.pop("flag_armed", False):  # the pinned word itself says when the copy has landed (`cap_flag_arm`)
                host = st["flag_host"]
                spins = 0
                t_w = time.perf_counter() if int(host.item()) < 0 else None  # (the host is AHEAD of the device here: waiting, not working)
                while int(host.item()) < 0:
                    spins += 1
                    if spins > 2_000_000:  # (never seen) not for ever on a lost copy: wait for the copy's event, read ONCE more
                        if ev is not None:
                            ev.synchronize()
                        else:
                            torch.cuda.current_stream(dev).synchronize()
                        if int(host.item()) < 0:
                            raise RuntimeError("capacity exchange: the overflow word's D2H copy completed without overwriting "
                                               "the host sentinel (flag_host still < 0)")
                        break
                if t_w is not None:
                    self.flag_wait_s += time.perf_counter() - t_w
            elif ev is not None:
                ev.synchronize()
            over = int(st.pop("flag_host").item())
            if over:
                self.exchange_stats["overflow_retries"] += 1
                return self.input_dist_end(self.input_dist_begin(st["kjt"], st["dst_names"], exact=True, slot=st["slot"]))
            self.exchange_stats["capacity_batches"] += 1
            return st
        if "rw_n" in rm and "recv_ids" not in st:
            if "counts_event" in st:
                st["counts_event"].synchronize()  # host sync: all-to-all split sizes live on the host
            both = st["counts_host"].view(2, W, rm["rw_n"]).sum(2)
            send_splits, recv_splits = both[0].tolist(), both[1].tolist()
            n_recv = int(sum(recv_splits))
            recv_ids = torch.empty(n_recv, dtype=torch.int64, device=dev)
            self._a2a(recv_ids, st["bkt_values"], recv_splits, send_splits)
            key_start = torch.zeros(W * rm["rw_n"] + 1, dtype=torch.int64, device=dev)
            torch.cumsum(st["recv_cnt"], 0, out=key_start[1:])
            st.update({"om": self._owner_meta(rm["rw_key_table"]), "recv_ids": recv_ids, "key_start": key_start,
                       "send_splits": send_splits, "recv_splits": recv_splits, "n_recv": n_recv})
        return st

    def lookup(self, st: dict, outs: Optional[List[torch.Tensor]] = None) -> List[torch.Tensor]:
        L = _lib.lib()
        dev, D = self._device, self.dim
        kjt, rm, uniform = st["kjt"], st["rm"], st["uniform"]
        B = kjt.stride()
        stream = _lib.stream_ptr(dev)
        if outs is None:
            outs = [torch.empty(B, w, dtype=torch.float32, device=dev) for w in rm["widths"]]
        dsts = self._dst_array(outs, B, rm["widths"])
        work = None
        if "rw_n" in rm:
            sub = st["sub"]
            F = rm["rw_n"]
            # rows back to the requesters (bucketized order) -- in flight while the replicas are read
            rows_in, d_pt, work = self.exchange_rows(st)
        if "dp_n" in rm:  # replicated tables: purely local, same destination buffers (other columns)
            if self._lookup_trackers:
                if "dp_track_segs" not in rm:
                    index = {k: i for i, k in enumerate(kjt.keys())}
                    dp = {c.name for c in self._dp}
                    rm["dp_track_segs"] = tuple((self._global[t].name, index[k]) for k, t, _ in self._lookups if self._global[t].name in dp)
                for fn in self._lookup_trackers:
                    fn(self, rm["dp_track_segs"], kjt.values(), None if uniform else kjt.offsets(), B, 1 if uniform else 0)
            _lib.check(L.tzr_pooled_fwd_ex(_lib.ptr(rm["dp_d_tables"]), _lib.ptr(rm["dp_d_feats"]), rm["dp_n"],
                                           _lib.ptr(rm["dp_d_slots"]), rm["dp_slots_n"], _lib.ptr(kjt.values()),
                                           _lib.ptr(None if uniform else kjt.offsets()), _lib.ptr(kjt.weights_or_none()),
                                           B, dsts, len(outs), 1 if uniform else 0,
                                           _lib.FWD_MIXED_DTYPE if self.replica._has_fp16 else 0, stream), "tzr_pooled_fwd")
        if work is not None:
            work.wait()
            # requester: pooled gather over the received rows, ids = position in bucketized order
            _lib.check(L.tzr_pooled_fwd(_lib.ptr(d_pt), _lib.ptr(rm["rw_d_feats"]), F, _lib.ptr(rm["rw_d_slots"]),
                                        rm["rw_slots_n"], _lib.ptr(st["unb"]), _lib.ptr(None if uniform else sub.offsets()),
                                        _lib.ptr(None if sub is None else sub.weights_or_none()), B, dsts, len(outs), 1 if uniform else 0,
                                        stream), "tzr_pooled_fwd")
        return outs

    def exchange_rows(self, st: dict):
        """Owner side of the forward: one embedding row per received id, sent back to the requesters.
        Returns (rows_in [N, D] in bucketized order, its one-table descriptor, the in-flight all-to-all)."""
        L, dev, D = _lib.lib(), self._device, self.dim
        om, n_recv = st["om"], st["n_recv"]
        F, N = st["rm"]["rw_n"], st["N_rw"]
        # ZCH tables: raw id -> row through the owner's map first
        st["owner_ids"] = st["recv_ids"] if self._owner_remap is None else self._owner_remap(st)
        if self._lookup_trackers and n_recv > 0:
            for fn in self._lookup_trackers:
                fn(self, om["track_segs"], st["owner_ids"], st["key_start"], 1, 0)
        rows_out = torch.empty(max(n_recv, 1), D, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_rows_gather(_lib.ptr(om["d_tables"]), _lib.ptr(om["d_key_table"]), _lib.ptr(st["key_start"]),
                                     om["K"], _lib.ptr(st["owner_ids"]), n_recv, _lib.ptr(rows_out), D, D,
                                     _lib.stream_ptr(dev)), "tzr_rows_gather")
        n_back = st.get("N_pad", N)  # capacity-bounded: rows come back in the fixed slices the ids left in
        rows_in, d_pt = self._recv_rows_buffer(n_back, F)
        work = self._a2a(rows_in[:n_back], rows_out[:n_recv], st["send_splits"], st["recv_splits"], async_op=True)
        return rows_in, d_pt, work

    # K6 depends on ids only: a pipeline may run both plans right after the input dist, one batch
    # ahead on its side stream (`plan_ahead`), and the backward then starts at K7
    def _dp_problem(self, st: dict) -> SparseBackward:
        """replicated tables: the pooled gradients of my samples, summed per row into `_dp_acc` (the accumulate descriptors)"""
        kjt, rm, uniform = st["kjt"], st["rm"], st["uniform"]
        B, N_all, n_dp = kjt.stride(), kjt.values().numel(), rm["dp_n"]
        return SparseBackward(self._device, rm["dp_d_acc_tables"], rm["dp_d_bwd_feats"], len(self._dp), n_dp, rm["n_keys"],
                              rm["dp_max_rows"], self.dim, kjt.values(), None if uniform else kjt.offsets(), kjt.weights_or_none(),
                              N_all, n_dp * B if uniform else N_all, B)

    def _rw_problem(self, st: dict) -> SparseBackward:
        """owned shards: one gradient row per received id, the ids of each (sender, key) segment behind `key_start`.  (ZCH tables:
        the row ids are the owner's remap of the received ones, which exists once `exchange_rows` has run.)"""
        om, n_recv = st["om"], st["n_recv"]
        return SparseBackward(self._device, om["d_bwd_tables"], om["d_bwd_feats"], om["T"], om["K"], om["K"], om["max_rows"], self.dim,
                              st.get("owner_ids", st["recv_ids"]), st["key_start"], None, n_recv, n_recv, 1, grad_mode=1)

    def _plan_half(self, st: dict, what: str, p: SparseBackward) -> torch.Tensor:
        ws = self._slot_workspace(st.get("slot") if "cap" in st else None, "ws_" + what, p.plan_bytes())
        p.plan(ws)
        return ws

    def _plan_dp(self, st: dict) -> torch.Tensor:
        return self._plan_half(st, "dp", self._dp_problem(st))

    def _plan_rw(self, st: dict) -> torch.Tensor:
        return self._plan_half(st, "rw", self._rw_problem(st))

    # -- the fused backward of one half (replicas / owned shards): planned pair, or ONE launch for small batches ------
    def _direct_ws(self, what: str, st: dict, p: SparseBackward) -> torch.Tensor:
        """persistent zero-initialised workspace of tzr_pooled_bwd_direct (its counters reset themselves); one per half,
        pipeline slot and size -- never evicted: captured graphs hold the address"""
        key = ("direct", what, st.get("slot") if "cap" in st else None, int(p.n_positions), int(p.n_tables))
        hit = self._slot_bufs.get(key)
        if hit is None:
            hit = self._slot_bufs[key] = _lib.zeroed_workspace(p.direct_bytes(), self._device)
        return hit

    # (sizes only: `plan_ahead` asks before the owner's row ids exist)
    def _dp_direct(self, st: dict) -> bool:
        kjt, n_dp = st["kjt"], st["rm"]["dp_n"]
        return direct_supported(n_dp * kjt.stride() if st["uniform"] else kjt.values().numel(), n_dp, len(self._dp), st["uniform"])

    def _rw_direct(self, st: dict) -> bool:
        return direct_supported(st["n_recv"], st["om"]["K"], st["om"]["T"], False, 1)

    def _bwd_half(self, st: dict, what: str, p: SparseBackward, grads, opt) -> None:
        if p.direct_supported():
            p.direct(self._direct_ws(what, st, p), grads, opt)
            return
        ws = st.get("ws_" + what)
        if ws is None:
            ws = st["ws_" + what] = self._plan_half(st, what, p)
        p.apply(ws, grads, opt)

    def _bwd_dp(self, st: dict, gd) -> None:
        """replicated tables: exact per-row gradient sums of my samples into `_dp_acc` (ACCUMULATE)"""
        dev = self._device
        # `_dp_acc` is zero on entry because the previous step's tzr_dense_rows_update_clear left it so.  A step that raised
        # between this pass and that update left sums behind: cleared here (never inside a capture: a captured step ran whole)
        if getattr(self, "_dp_acc_dirty", False) and not (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            self._dp_acc.zero_()
        self._dp_acc_dirty = True
        self._bwd_half(st, "dp", self._dp_problem(st), gd, self._optim_struct(_lib.OPT_ACCUMULATE))

    def _bwd_rw(self, st: dict, grecv: torch.Tensor) -> None:
        """owned shards: sort by (table, row) + fused optimizer over the received per-id gradient rows"""
        if st["n_recv"] <= 0:
            return
        self._bwd_half(st, "rw", self._rw_problem(st), grad_dsts([grecv]), self._optim_struct())

    def plan_ahead(self, st: dict) -> dict:
        """K6 of both halves, for a pipeline to run a batch ahead -- for the halves that have a plan at all (a small
        batch's backward is one launch without one: `_dp_direct` / `_rw_direct`)"""
        if self.fused_optimizer is not None:
            if "dp_n" in st["rm"] and not self._dp_direct(st):
                st["ws_dp"] = self._plan_dp(st)
            # (hash-routed tables: the row ids only exist after the owner's remap in `lookup`)
            if "rw_n" in st["rm"] and st.get("n_recv", 0) > 0 and self._owner_remap is None and not self._rw_direct(st):
                st["ws_rw"] = self._plan_rw(st)
        return st

    def _forward_impl(self, kjt: KeyedJaggedTensor, dst_names):
        # (a lone forward checks the overflow word right away: the same host wait the exact exchange has)
        st = self.input_dist_end(self.input_dist_begin(kjt, dst_names))
        return self.lookup(st), st

    def backward(self, st: dict, grads: Sequence[Optional[torch.Tensor]]) -> None:
        """Fused sparse optimizer step for the lookups of `st` given the pooled-output gradients."""
        self._backward_impl(st, grads)

    def _backward_impl(self, st, grads, id_grads: Optional[torch.Tensor] = None) -> None:
        """`grads`: gradients of the pooled outputs; or `id_grads` [N, D]: one gradient row per exchanged
        lookup, already in bucketized order (the unpooled / sequence lookup)."""
        if self.fused_optimizer is None:
            return
        L = _lib.lib()
        dev, D = self._device, self.dim
        self.fused_optimizer.begin_step(dev)  # Adam's step counter: once for the row-wise and the replicated tables
        kjt, rm, uniform = st["kjt"], st["rm"], st["uniform"]
        B = kjt.stride()
        stream = _lib.stream_ptr(dev)
        gl = []
        for g, w in zip(grads, rm["widths"]):
            if g is None:
                g = torch.zeros(B, w, dtype=torch.float32, device=dev)
            gl.append(g.contiguous().float())
        gd = grad_dsts(gl)

        # Order of issue = overlap: the gradient all-to-all flies while the replicas' gradients are
        # sorted and summed; their all-reduce flies while the owners sort and apply the exchanged rows.
        w_rows = w_acc = None
        if "rw_n" in rm:
            om, sub, n_recv = st["om"], st["sub"], st["n_recv"]
            N, F = st["N_rw"], rm["rw_n"]
            # requester: one gradient row per id, in bucketized order -> to the owners
            n_out = st.get("N_pad", N)
            if id_grads is not None:
                if n_out != N:
                    raise ValueError("per-id gradients go through the exact exchange")
                grow = id_grads
            else:
                grow = torch.empty(max(n_out, 1), D, dtype=torch.float32, device=dev)
                _lib.check(L.tzr_lookup_grads(_lib.ptr(rm["rw_d_feats"]), F, _lib.ptr(None if uniform else sub.offsets()),
                                              _lib.ptr(None if sub is None else sub.weights_or_none()), B, 1 if uniform else 0, _lib.ptr(st["unb"]),
                                              gd, len(gl), _lib.ptr(grow), D, D, stream), "tzr_lookup_grads")
            grecv = torch.empty(max(n_recv, 1), D, dtype=torch.float32, device=dev)
            w_rows = self._a2a(grecv[:n_recv], grow[:n_out], st["recv_splits"], st["send_splits"], async_op=True)
        if "dp_n" in rm:
            # replicas: exact per-row gradient sums of my samples -> all-reduce -> same dense update
            self._bwd_dp(st, gd)  # (`_dp_acc` is zero: tzr_dense_rows_update_clear leaves it so)
            w_acc = dist.all_reduce(self._dp_acc, group=self.pg, async_op=True)
        if w_rows is not None:
            w_rows.wait()
            # owner: sort by (table,row) + fused optimizer, gradients addressed per id
            self._bwd_rw(st, grecv)
        if w_acc is not None:
            w_acc.wait()
            _lib.check(L.tzr_dense_rows_update_clear(_lib.ptr(rm["dp_d_tables"]), len(self._dp), _lib.ptr(self._dp_row_start),
                                               self._dp_rows, _lib.ptr(self._dp_acc), D, self._optim_struct(), stream),
                       "tzr_dense_rows_update_clear")
            self._dp_acc_dirty = False
        self._after_backward(st)

    def _after_backward(self, st: dict) -> None:
        pass

    # -- the step cut at its collectives ---------------------------------------------------------------------
    # `ShardedTrainStep(step_graph=True)`: every `seg_*` below is kernels on static buffers only (one hipGraph per
    # run of them), every `coll_*` is the RCCL calls between two such runs, issued eagerly (RCCL kernels captured
    # into a hipGraph took the process down at hipStreamEndCapture on this stack: profiles/r02p).  Same kernels,
    # same arguments, same order per table as `lookup` / `_backward_impl`; only the overlap of a collective with the
    # replicas' kernels is given up.  Capacity-bounded states only (`"cap" in st`).
    def _dst_array(self, outs: Sequence[torch.Tensor], B: int, widths: Sequence[int]):
        for o, w in zip(outs, widths):
            if o.shape != (B, w) or o.stride(1) != 1:
                raise ValueError("output buffer shape")
        return grad_dsts(outs)

    def seg_owner_rows(self, st: dict, outs: List[torch.Tensor], dp: bool = True) -> None:
        """owner: one row per received id (-> `coll_rows`); `dp`: also the replicated tables, pooled straight into `outs`
        (`seg_dp_pool`; a pipeline that issues the rows all-to-all async runs that half BEHIND the issue instead)"""
        L, dev, D = _lib.lib(), self._device, self.dim
        kjt, rm = st["kjt"], st["rm"]
        stream = _lib.stream_ptr(dev)
        if "rw_n" in rm:
            om, n_recv = st["om"], st["n_recv"]
            st["owner_ids"] = st["recv_ids"]
            for fn in self._lookup_trackers:
                fn(self, om["track_segs"], st["owner_ids"], st["key_start"], 1, 0)
            st["rows_out"] = self._slot(st["slot"], "rows_out", (n_recv, D), torch.float32)
            _lib.check(L.tzr_rows_gather(_lib.ptr(om["d_tables"]), _lib.ptr(om["d_key_table"]), _lib.ptr(st["key_start"]),
                                         om["K"], _lib.ptr(st["owner_ids"]), n_recv, _lib.ptr(st["rows_out"]), D, D, stream),
                       "tzr_rows_gather")
        if dp:
            self.seg_dp_pool(st, outs)

    def seg_dp_pool(self, st: dict, outs: List[torch.Tensor]) -> None:
        """replicated tables: purely local pooled lookup, straight into their columns of `outs`"""
        L, dev = _lib.lib(), self._device
        kjt, rm = st["kjt"], st["rm"]
        B, stream = kjt.stride(), _lib.stream_ptr(dev)
        if "dp_n" in rm:
            if self._lookup_trackers:
                if "dp_track_segs" not in rm:
                    index = {k: i for i, k in enumerate(kjt.keys())}
                    dp = {c.name for c in self._dp}
                    rm["dp_track_segs"] = tuple((self._global[t].name, index[k]) for k, t, _ in self._lookups if self._global[t].name in dp)
                for fn in self._lookup_trackers:
                    fn(self, rm["dp_track_segs"], kjt.values(), None, B, 1)
            _lib.check(L.tzr_pooled_fwd_ex(_lib.ptr(rm["dp_d_tables"]), _lib.ptr(rm["dp_d_feats"]), rm["dp_n"],
                                           _lib.ptr(rm["dp_d_slots"]), rm["dp_slots_n"], _lib.ptr(kjt.values()), None,
                                           None, B, self._dst_array(outs, B, rm["widths"]), len(outs), 1,
                                           _lib.FWD_MIXED_DTYPE if self.replica._has_fp16 else 0, stream), "tzr_pooled_fwd")

    def coll_rows(self, st: dict, async_op: bool = False):
        """the rows all-to-all; `async_op`: returns the work handle (the caller's stream waits on `.wait()`)"""
        if "rw_n" in st["rm"]:
            rows_in, _ = self._recv_rows_buffer(st["N_pad"], st["rm"]["rw_n"])
            if async_op:
                return a2a_async(rows_in[:st["N_pad"]], st["rows_out"], self.pg)
            return stream_collective(dist.all_to_all_single, rows_in[:st["N_pad"]], st["rows_out"], group=self.pg)
        return None

    def seg_pool(self, st: dict, outs: List[torch.Tensor]) -> None:
        """requester: pooled gather over the rows that came back (ids = their positions in the message)"""
        rm = st["rm"]
        if "rw_n" in rm:
            B, F = st["kjt"].stride(), rm["rw_n"]
            _, d_pt = self._recv_rows_buffer(st["N_pad"], F)
            _lib.check(_lib.lib().tzr_pooled_fwd(_lib.ptr(d_pt), _lib.ptr(rm["rw_d_feats"]), F, _lib.ptr(rm["rw_d_slots"]),
                                                 rm["rw_slots_n"], _lib.ptr(st["unb"]), None, None, B,
                                                 self._dst_array(outs, B, rm["widths"]), len(outs), 1,
                                                 _lib.stream_ptr(self._device)), "tzr_pooled_fwd")

    def seg_grads(self, st: dict, grads: Sequence[torch.Tensor]) -> None:
        """requester: one gradient row per id into the message layout (-> `coll_grads`); replicas: row sums"""
        self.seg_grads_rw(st, grads)
        self.seg_grads_dp(st)

    def seg_grads_rw(self, st: dict, grads: Sequence[torch.Tensor]) -> None:
        """first half of `seg_grads`: the per-id gradient rows (everything the gradient all-to-all waits for)"""
        if self.fused_optimizer is None:
            return
        L, dev, D = _lib.lib(), self._device, self.dim
        self.fused_optimizer.begin_step(dev)
        kjt, rm = st["kjt"], st["rm"]
        B, stream = kjt.stride(), _lib.stream_ptr(dev)
        gl = [g.contiguous().float() for g in grads]
        st["_grads_alive"] = gl
        if "rw_n" in rm:
            gd = self._dst_array(gl, B, rm["widths"])
            st["grow"] = self._slot(st["slot"], "grow", (st["N_pad"], D), torch.float32)
            _lib.check(L.tzr_lookup_grads(_lib.ptr(rm["rw_d_feats"]), rm["rw_n"], None, None, B, 1, _lib.ptr(st["unb"]), gd, len(gl),
                                          _lib.ptr(st["grow"]), D, D, stream), "tzr_lookup_grads")

    def seg_grads_dp(self, st: dict) -> None:
        """second half: the replicated tables' exact per-row gradient sums of my samples (-> their all-reduce)"""
        if self.fused_optimizer is None:
            return
        L, dev, D = _lib.lib(), self._device, self.dim
        kjt, rm = st["kjt"], st["rm"]
        B, stream = kjt.stride(), _lib.stream_ptr(dev)
        if "dp_n" in rm:
            gl = st["_grads_alive"]
            gd = self._dst_array(gl, B, rm["widths"])
            self._bwd_dp(st, gd)  # (`_dp_acc` is zero: tzr_dense_rows_update_clear leaves it so)

    def coll_grads(self, st: dict) -> None:
        self.coll_grads_rw(st)
        self.coll_grads_dp(st)

    def coll_grads_rw(self, st: dict, async_op: bool = False):
        """the gradient all-to-all; `async_op`: returns the work handle (the caller's stream waits on `.wait()`)"""
        if self.fused_optimizer is None or "rw_n" not in st["rm"]:
            return None
        st["grecv"] = self._slot(st["slot"], "grecv", (st["n_recv"], self.dim), torch.float32)
        if async_op:
            return a2a_async(st["grecv"], st["grow"], self.pg)
        return stream_collective(dist.all_to_all_single, st["grecv"], st["grow"], group=self.pg)

    def coll_grads_dp(self, st: dict, async_op: bool = False):
        """the all-reduce of the replicated tables' row sums"""
        if self.fused_optimizer is None or "dp_n" not in st["rm"]:
            return None
        if async_op:
            return allreduce_async(self._dp_acc, self.pg)
        return stream_collective(dist.all_reduce, self._dp_acc, group=self.pg)

    def seg_apply(self, st: dict) -> None:
        """owner: sort + fused optimizer over the received gradient rows; replicas: the dense row update"""
        self.seg_apply_rw(st)
        self.seg_apply_dp(st)

    def seg_apply_rw(self, st: dict) -> None:
        """first half of `seg_apply`: needs the gradient all-to-all only"""
        if self.fused_optimizer is None:
            return
        L, dev, D = _lib.lib(), self._device, self.dim
        rm, stream = st["rm"], _lib.stream_ptr(dev)
        if "rw_n" in rm:
            self._bwd_rw(st, st["grecv"])

    def seg_apply_dp(self, st: dict) -> None:
        """second half: needs the all-reduced row sums of the replicated tables"""
        if self.fused_optimizer is None:
            return
        L, dev, D = _lib.lib(), self._device, self.dim
        rm, stream = st["rm"], _lib.stream_ptr(dev)
        if "dp_n" in rm:
            _lib.check(L.tzr_dense_rows_update_clear(_lib.ptr(rm["dp_d_tables"]), len(self._dp), _lib.ptr(self._dp_row_start),
                                               self._dp_rows, _lib.ptr(self._dp_acc), D, self._optim_struct(), stream),
                       "tzr_dense_rows_update_clear")
            self._dp_acc_dirty = False
        self._after_backward(st)

    # -- public API ------------------------------------------------------------------------------
    def forward_grouped(self, features: KeyedJaggedTensor, group_names=None) -> Dict[str, torch.Tensor]:
        names = tuple(group_names) if group_names is not None else tuple(self._groups)
        if torch.is_grad_enabled() and self.fused_optimizer is not None and self.training:
            outs = list(_ShardedLookupFn.apply(self, features, names, self._hook))
        else:
            outs, _ = self._forward_impl(features, names)
        return dict(zip(names, outs))


def allreduce_average(grads: Sequence[torch.Tensor], process_group=None) -> None:
    """Average `grads` over the ranks in place: pack, ONE all-reduce, unpack (3 launches)."""
    gs = [g for g in grads if g is not None]
    if not gs:
        return
    world = dist.get_world_size(process_group)
    flat = torch.cat([g.reshape(-1) for g in gs])
    if flat.is_cuda:
        stream_collective(dist.all_reduce, flat, op=dist.ReduceOp.AVG, group=process_group)
    else:  # gloo has no AVG
        dist.all_reduce(flat, group=process_group)
        flat.div_(world)
    torch._foreach_copy_(gs, [c.view_as(g) for c, g in zip(flat.split([g.numel() for g in gs]), gs)])


class ShardedDLRM(nn.Module):
    """DLRM with sharded tables and data-parallel MLPs."""

    def __init__(self, tables, sparse_features, dense_dim, dense_mlp=(64, 16), final_mlp=(64, 32),
                 arch_with_sparse=True, device=None, sparse_optimizer=None, row_layout="interleaved",
                 process_group=None, dp_max_rows: int = 65536, replicate_at_world1: bool = False,
                 constraints: Optional[Dict[str, str]] = None, tw_max_rows: int = 0,
                 plan: Optional[Dict[str, dict]] = None, exchange: str = "exact", capacity_factor: float = 1.25) -> None:
        super().__init__()
        self.pg = process_group
        self.dim = tables[0].embedding_dim
        self.num_sparse = len(sparse_features)
        self.arch_with_sparse = arch_with_sparse
        self.ebc = ShardedEmbeddingBagCollection(
            tables, device=device, optimizer=sparse_optimizer, groups={"sparse": list(sparse_features)},
            row_layout=row_layout, process_group=process_group, dp_max_rows=dp_max_rows,
            replicate_at_world1=replicate_at_world1, constraints=constraints, tw_max_rows=tw_max_rows, plan=plan,
            exchange=exchange, capacity_factor=capacity_factor)
        self.dense_mlp = MLP(dense_dim, dense_mlp).to(device)
        n = self.num_sparse + 1
        feat = n * (n - 1) // 2 + self.dim + (self.num_sparse * self.dim if arch_with_sparse else 0)
        self.final_mlp = MLP(feat, final_mlp).to(device)
        self.output_mlp = OutputLinear(final_mlp[-1], 1).to(device)
        # the bottom MLP does not depend on the exchange: on a GPU it runs on a second HIP stream
        # while the id / row all-to-alls are in flight
        self.overlap_dense = True
        self._side: Optional[torch.cuda.Stream] = None
        # same dense parameters on every rank (DDP broadcasts rank 0's at construction)
        for p in self.dense_parameters():
            stream_collective(dist.broadcast, p.data, src=0, group=self.pg)

    def describe(self) -> str:
        e = self.ebc
        n_tw = sum(1 for p in e._plan.values() if p["sharding_type"] == "table_wise")
        return (f"{e.W} ranks: {len(e._rw) - n_tw} tables row-wise (block=ceil(rows/{e.W})) + {n_tw} table-wise (id-granularity all-to-all of "
                f"ids/rows/grads over RCCL), {len(e._dp)} small tables data_parallel (local lookup, one all-reduce of "
                f"row gradients); MLPs data-parallel with all-reduce")

    def dense_parameters(self):
        for m in (self.dense_mlp, self.final_mlp, self.output_mlp):
            yield from m.parameters()

    def dense_forward(self, dense: torch.Tensor, sparse: torch.Tensor) -> torch.Tensor:
        """Everything after the lookup: bottom MLP, dot interaction, top MLP -> logits [B]."""
        d = self.dense_mlp(dense)
        allf = dot_interaction(d, sparse, self.dim, cat_dense=True, cat_sparse=self.arch_with_sparse)
        return self.output_mlp(self.final_mlp(allf)).squeeze(1)

    def dense_loss(self, dense: torch.Tensor, sparse: torch.Tensor, labels: torch.Tensor, d: Optional[torch.Tensor] = None):
        """(mean BCE-with-logits loss over this rank's samples, logits [B]): `dense_forward` + the loss with everything
        behind the top MLP's first GEMM in one launch when the stack fits (torcheasyrec_amd.dense.top_loss; the
        unsharded DLRM.loss_from_embeddings does the same)."""
        from .dlrm import head_loss

        return head_loss(self, dense, sparse, labels, d=d)

    def dense_bottom(self, dense: torch.Tensor) -> torch.Tensor:
        """the bottom MLP alone: the one piece of the dense half that does not depend on the exchange -- a pipeline runs
        it while the rows all-to-all is in flight and hands the result to `dense_loss(..., d=)`"""
        return self.dense_mlp(dense)

    def forward(self, dense: torch.Tensor, sparse_features: KeyedJaggedTensor) -> torch.Tensor:
        if dense.is_cuda and self.overlap_dense:
            cur = torch.cuda.current_stream(dense.device)
            if self._side is None:
                self._side = torch.cuda.Stream(dense.device)
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                d = self.dense_mlp(dense)  # autograd replays its backward on the same side stream
            sparse = self.ebc.forward_grouped(sparse_features)["sparse"]
            cur.wait_stream(self._side)
            d.record_stream(cur)
        else:
            sparse = self.ebc.forward_grouped(sparse_features)["sparse"]
            d = self.dense_mlp(dense)
        allf = dot_interaction(d, sparse, self.dim, cat_dense=True, cat_sparse=self.arch_with_sparse)
        return self.output_mlp(self.final_mlp(allf)).squeeze(1)

    def forward_loss(self, dense: torch.Tensor, sparse_features: KeyedJaggedTensor, labels: torch.Tensor):
        """(loss, logits): the op-by-op training forward with the same loss path as the pipelined step (`dense_loss`)."""
        sparse = self.ebc.forward_grouped(sparse_features)["sparse"]
        return self.dense_loss(dense, sparse, labels)

    def allreduce_dense_grads(self, grads: Optional[Sequence[torch.Tensor]] = None) -> None:
        """DDP semantics: average dense gradients over ranks -- one flat all-reduce (217 KB), three
        launches (pack, all-reduce, unpack)."""
        gs = list(grads) if grads is not None else [p.grad for p in self.dense_parameters() if p.grad is not None]
        if not gs:
            return
        world = dist.get_world_size(self.pg)
        flat = torch.cat([g.reshape(-1) for g in gs])
        if flat.is_cuda:
            stream_collective(dist.all_reduce, flat, op=dist.ReduceOp.AVG, group=self.pg)
        else:  # gloo has no AVG
            dist.all_reduce(flat, group=self.pg)
            flat.div_(world)
        torch._foreach_copy_(gs, [c.view_as(g) for c, g in zip(flat.split([g.numel() for g in gs]), gs)])


def pack_dense_grads(grads: Sequence[torch.Tensor]) -> torch.Tensor:
    """the flat buffer of the dense all-reduce.  On the library's device: one launch that takes every gradient as it lies (partial
    sums a backward left behind for FusedDenseAdam(fuse_finish=True) are added up on the way in -- no finishing launches, no
    concatenation: four launches fewer per step of the DLRM model)."""
    from .dense import materialize_pending, pack_gradients

    grads = list(grads)
    if grads and (grads[0].is_cuda or _lib.emulated(load=True)):
        flat = pack_gradients(grads)
        if flat is not None:
            return flat
    materialize_pending(grads)  # (the collective wants tensors)
    return torch.cat([g.reshape(-1) for g in grads])


def allreduce_flat_average(flat: torch.Tensor, process_group=None, async_op: bool = False):
    if flat.is_cuda:
        if async_op:
            return allreduce_async(flat, process_group, avg=True)
        return stream_collective(dist.all_reduce, flat, op=dist.ReduceOp.AVG, group=process_group)
    # gloo has no AVG (and nothing to overlap with on the CPU: always finished on return)
    dist.all_reduce(flat, group=process_group)
    flat.div_(dist.get_world_size(process_group))
    return None


def unpack_dense_grads(flat: torch.Tensor, grads: Sequence[torch.Tensor]) -> None:
    torch._foreach_copy_(list(grads), [c.view_as(g) for c, g in zip(flat.split([g.numel() for g in grads]), grads)])


def dense_grad_views(flat: torch.Tensor, grads: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """The averaged gradients where they already are: contiguous views of the all-reduced flat buffer, shaped like
    `grads` -- what `unpack_dense_grads` would copy out (one multi-tensor launch, 14.5 us for DLRM's ten tensors,
    profiles/r03bv/kernel_stats_8192.csv) for an optimizer that reads them once."""
    return [c.view_as(g) for c, g in zip(flat.split([g.numel() for g in grads]), grads)]


def _column_shards(dim: int, world: int) -> int:
    """Default number of column shards of a `column_wise` table: the largest k <= world with dim / k a
    multiple of 4 (the kernels' float4 granularity)."""
    q = dim // 4
    return max(k for k in range(1, min(world, q) + 1) if q % k == 0)


class _MixedLookupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, kjt, dst_names, hook):
        outs, states = mod._forward_impl(kjt, dst_names)
        ctx.mod, ctx.states = mod, states
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        ctx.mod._backward_impl(ctx.states, grads)
        return None, None, None, None


class MixedShardedEmbeddingBagCollection(nn.Module):
    """Sharded pooled lookup without the two restrictions of `ShardedEmbeddingBagCollection` -- tables
    of several embedding dims (DeepFM: wide + deep tables) and features that feed more than one table --
    plus `column_wise` sharding (/root/reference/tzrec/protos/feature.proto:8; torchrec splits a
    table's columns into shards that live on different ranks, every shard owner serves every id of the
    feature and the requester concatenates the pieces).

    Built from what is there: the id-granularity exchange moves fixed-width rows, so the tables are
    split into LANES -- one `ShardedEmbeddingBagCollection` per (embedding dim, no feature twice) --
    that all write their blocks into the same feature-group buffers.  A `column_wise` table of dim D
    with k shards becomes k table-wise tables `<name>@cw<j>` of dim D/k (same rows, same ids, columns
    [j*D/k, (j+1)*D/k) of the table and of its initialiser), placed on different ranks; its pooled
    block is the concatenation of the k pieces, which is simply where the k lanes write.  Each lane
    runs its own id / row all-to-alls (k column shards of one feature are k lanes): column-wise is
    for the few tables that are too wide for one rank's link, not for everything.

    `plan[table]["sharding_type"] == "column_wise"` (with `ranks` = owner of every column shard) or
    `constraints[table] = "column_wise"` selects it.  torchrec's hierarchical types are accepted with their
    single-node meaning: `table_row_wise` = `row_wise`, `table_column_wise` = `column_wise`, `grid_shard` =
    column shards that are each row-wise over the node's ranks.  `forward_grouped` / `fused_optimizer` /
    `table_weights` / `plan` as in the one-dim collection; the three-phase pipeline API is per lane."""

    def __init__(self, tables: Sequence[EmbeddingBagConfig], device: torch.device, optimizer: Optional[SparseOptimizerConfig] = None,
                 groups: Optional[Dict[str, List[str]]] = None, row_layout: str = "interleaved",
                 process_group: Optional[dist.ProcessGroup] = None, dp_max_rows: int = 65536,
                 constraints: Optional[Dict[str, str]] = None, tw_max_rows: int = 0,
                 plan: Optional[Dict[str, dict]] = None, exchange: str = "exact", capacity_factor: float = 1.25) -> None:
        super().__init__()
        self.pg = process_group
        self.W, self.rank = dist.get_world_size(self.pg), dist.get_rank(self.pg)
        self._device = torch.device(device)
        self._tables = list(tables)
        constraints = dict(constraints or {})
        feat_tables: Dict[str, List[str]] = {}
        for cfg in self._tables:
            for f in cfg.feature_names:
                feat_tables.setdefault(f, []).append(cfg.name)
        # block names of the user's groups: feature, or feature@table when the feature feeds > 1 table
        # (the unsharded collection's rule, tzrec/modules/embedding.py:753-758,826-827)
        block_of = {(f, cfg.name): (f if len(feat_tables[f]) == 1 else f"{f}@{cfg.name}") for cfg in self._tables for f in cfg.feature_names}
        # -- column-wise tables -> table-wise column shards ----------------------------------------
        self._cw: Dict[str, List[str]] = {}
        self._grid: set = set()
        virt: List[EmbeddingBagConfig] = []
        v_constraints: Dict[str, str] = {}
        v_plan: Optional[Dict[str, dict]] = {} if plan is not None else None
        pieces: Dict[str, List[Tuple[str, int]]] = {}  # user block -> [(lane block, width)]
        v_out_keys: Dict[Tuple[str, str], str] = {}
        for cfg in self._tables:
            entry = plan.get(cfg.name) if plan is not None else None
            if plan is not None and entry is None:
                raise ValueError(f"sharding plan has no entry for {cfg.name}")
            kind = entry["sharding_type"] if entry is not None else constraints.get(cfg.name)
            # torchrec's hierarchical types on ONE node (every rank is a local rank): table_row_wise = rows of a
            # table over the ranks of its host = row_wise; table_column_wise = column shards on the ranks of one
            # host = column_wise; grid_shard = column shards, each row-wise over a host = column shards that are
            # row-wise tables instead of table-wise ones (feature.proto:8)
            grid = kind == "grid_shard"
            if kind == "table_row_wise":
                kind = "row_wise"
                if entry is not None:
                    entry = dict(entry, sharding_type="row_wise", block=entry.get("block", max(1, -(-cfg.num_embeddings // self.W))),
                                 rot=entry.get("rot", 0), ranks=entry.get("ranks", list(range(self.W))))
                else:
                    constraints[cfg.name] = "row_wise"
            if kind in ("table_column_wise", "grid_shard"):
                kind = "column_wise"
            if kind == "column_wise":
                D = cfg.embedding_dim
                if entry is not None and entry.get("shard_dim"):
                    k = D // int(entry["shard_dim"])
                elif entry is not None and entry.get("ranks") and not grid:
                    k = len(entry["ranks"])
                else:
                    k = _column_shards(D, self.W)
                if k < 1 or D % k or (D // k) % 4:
                    raise ValueError(f"{cfg.name}: {k} column shards of a dim-{D} table (shard width must be a multiple of 4)")
                d = D // k
                self._cw[cfg.name] = []
                if grid:
                    self._grid.add(cfg.name)
                for j in range(k):
                    def init(w, cfg=cfg, j=j, d=d):  # noqa: E306
                        full = torch.empty(cfg.num_embeddings, cfg.embedding_dim)
                        if cfg.init_fn is not None:
                            cfg.init_fn(full)
                        else:
                            a = (1.0 / max(cfg.num_embeddings, 1)) ** 0.5
                            full.uniform_(-a, a)
                        w.copy_(full[:, j * d:(j + 1) * d])
                    name = f"{cfg.name}@cw{j}"
                    virt.append(EmbeddingBagConfig(name, d, cfg.num_embeddings, list(cfg.feature_names), cfg.pooling, init,
                                                   trainable=cfg.trainable, data_type=cfg.data_type))
                    self._cw[cfg.name].append(name)
                    if grid:  # every column shard is itself row-wise over the node
                        if v_plan is not None:
                            v_plan[name] = {"sharding_type": "row_wise", "block": max(1, -(-cfg.num_embeddings // self.W)), "rot": 0,
                                            "ranks": list(range(self.W))}
                        else:
                            v_constraints[name] = "row_wise"
                    elif v_plan is not None:
                        v_plan[name] = {"sharding_type": "table_wise", "block": cfg.num_embeddings, "rot": int(entry["ranks"][j]),
                                        "ranks": [int(entry["ranks"][j])]}
                    else:
                        v_constraints[name] = "table_wise"
                    for f in cfg.feature_names:
                        v_out_keys[(f, name)] = f"{block_of[(f, cfg.name)]}@cw{j}"
                        pieces.setdefault(block_of[(f, cfg.name)], []).append((v_out_keys[(f, name)], d))
            else:
                virt.append(cfg)
                if v_plan is not None:
                    v_plan[cfg.name] = entry
                elif cfg.name in constraints:
                    v_constraints[cfg.name] = constraints[cfg.name]
                for f in cfg.feature_names:
                    v_out_keys[(f, cfg.name)] = block_of[(f, cfg.name)]
                    pieces[block_of[(f, cfg.name)]] = [(block_of[(f, cfg.name)], cfg.embedding_dim)]
        if v_plan is None:  # ONE placement over everything, so the lanes balance together
            v_plan = make_plan(virt, self.W, dp_max_rows, False, v_constraints, tw_max_rows)
        self._virt = virt
        self._global = virt  # what `plan()` / `shard_of` / `table_weights` are keyed by (checkpoint.py reads it)
        self._vplan = v_plan
        # -- lanes: same dim, no feature twice --------------------------------------------------------
        lanes: List[List[EmbeddingBagConfig]] = []
        for cfg in virt:
            for lane in lanes:
                if lane[0].embedding_dim == cfg.embedding_dim and not (set(cfg.feature_names) & {f for c in lane for f in c.feature_names}):
                    lane.append(cfg)
                    break
            else:
                lanes.append([cfg])
        out_dims = {blk: w for ps in pieces.values() for blk, w in ps}
        self._user_groups = groups
        lane_groups = None if groups is None else {g: [blk for k in ks for blk, _ in pieces[k]] for g, ks in groups.items()}
        self._widths = None if groups is None else {g: sum(w for k in ks for _, w in pieces[k]) for g, ks in groups.items()}
        self._all_blocks = [blk for cfg in self._tables for f in cfg.feature_names for blk, _ in pieces[block_of[(f, cfg.name)]]]
        self._all_width = sum(out_dims[b] for b in self._all_blocks)
        self._block_of, self._pieces = block_of, pieces
        self.lanes = nn.ModuleList()
        for lane in lanes:
            names = {c.name for c in lane}
            g = dict(lane_groups) if lane_groups is not None else {}
            g["__mixed_all__"] = self._all_blocks  # table-then-feature order of the GLOBAL config list
            self.lanes.append(ShardedEmbeddingBagCollection(
                lane, device=self._device, optimizer=optimizer, groups=g, row_layout=row_layout, process_group=self.pg,
                plan={n: p for n, p in v_plan.items() if n in names},
                out_keys={k: v for k, v in v_out_keys.items() if k[1] in names}, out_dims=out_dims,
                exchange=exchange, capacity_factor=capacity_factor))
        self.fused_optimizer = self.lanes[0].fused_optimizer
        for lane in list(self.lanes)[1:]:  # one lr handle drives every lane
            if lane.fused_optimizer is not None:
                lane.fused_optimizer.param_groups = self.fused_optimizer.param_groups
                for part in (lane.local, lane.replica):
                    if part is not None and part.fused_optimizer is not None:
                        part.fused_optimizer.param_groups = self.fused_optimizer.param_groups
        self._hook = torch.zeros(0, requires_grad=True, device=self._device)

    # -- placement / state -------------------------------------------------------------------------
    def plan(self) -> Dict[str, dict]:
        """The plan the lanes execute (and checkpoints persist): a column-wise table appears as its
        table-wise column shards `<name>@cw<j>`; `_global` lists the same tables."""
        return self._vplan

    def sharding_plan(self) -> Dict[str, dict]:
        """Per configured table, torchrec's fields: column-wise tables as ONE entry with the owner rank of
        every column shard (tzrec/utils/checkpoint_util.py:1152-1167)."""
        out = {}
        for cfg in self._tables:
            if cfg.name in self._cw:
                shards = self._cw[cfg.name]
                if cfg.name in self._grid:
                    out[cfg.name] = {"sharding_type": "grid_shard", "ranks": list(range(self.W)), "shard_dim": cfg.embedding_dim // len(shards)}
                else:
                    out[cfg.name] = {"sharding_type": "column_wise", "ranks": [self._vplan[s]["ranks"][0] for s in shards],
                                     "shard_dim": cfg.embedding_dim // len(shards)}
            else:
                out[cfg.name] = self._vplan[cfg.name]
        return out

    def column_shards(self, name: str) -> List[str]:
        """Names of the column shards of a column-wise table, in column order (keys of `table_weights`)."""
        return list(self._cw[name])

    def _lane_of(self, name: str) -> ShardedEmbeddingBagCollection:
        return next(lane for lane in self.lanes if any(c.name == name for c in lane._global))

    def shard_of(self, name: str) -> Tuple[int, int]:
        return self._lane_of(name).shard_of(name)

    def table_weights(self) -> Dict[str, torch.Tensor]:
        out = {}
        for lane in self.lanes:
            out.update(lane.table_weights())
        return out

    def table_states(self) -> Dict[str, torch.Tensor]:
        out = {}
        for lane in self.lanes:
            out.update(lane.table_states())
        return out

    # -- lookup ----------------------------------------------------------------------------------------
    def _forward_impl(self, kjt: KeyedJaggedTensor, dst_names):
        B = kjt.stride()
        widths = [self._all_width if n == "__mixed_all__" else self._widths[n] for n in dst_names]
        outs = [torch.empty(B, w, dtype=torch.float32, device=self._device) for w in widths]
        # every lane's input dist first (their count exchanges and host syncs back to back), then the lookups
        states = [lane.input_dist_begin(kjt, dst_names) for lane in self.lanes]
        states = [lane.input_dist_end(st) for lane, st in zip(self.lanes, states)]
        for lane, st in zip(self.lanes, states):
            lane.lookup(st, outs)
        return outs, states

    def _backward_impl(self, states, grads) -> None:
        for lane, st in zip(self.lanes, states):
            lane._backward_impl(st, grads)

    def _run(self, features: KeyedJaggedTensor, names: Tuple[str, ...]) -> List[torch.Tensor]:
        for lane in self.lanes:
            lane.train(self.training)
        if torch.is_grad_enabled() and self.fused_optimizer is not None and self.training:
            return list(_MixedLookupFn.apply(self, features, names, self._hook))
        return self._forward_impl(features, names)[0]

    def forward_grouped(self, features: KeyedJaggedTensor, group_names=None) -> Dict[str, torch.Tensor]:
        if self._user_groups is None:
            raise ValueError("MixedShardedEmbeddingBagCollection was built without groups")
        names = tuple(group_names) if group_names is not None else tuple(self._user_groups)
        return dict(zip(names, self._run(features, names)))

    def forward(self, features: KeyedJaggedTensor):
        """KeyedTensor [B, sum D] in table-then-feature order, blocks named like the unsharded collection's."""
        from .sparse import KeyedTensor

        (out,) = self._run(features, ("__mixed_all__",))
        keys = [self._block_of[(f, cfg.name)] for cfg in self._tables for f in cfg.feature_names]
        return KeyedTensor(keys, [cfg.embedding_dim for cfg in self._tables for _ in cfg.feature_names], out)
