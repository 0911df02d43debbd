"""Sequence-embedding path (BASELINE config 4, multi_tower_din).

Mirrors the pieces of ``SequenceEmbeddingGroupImpl`` the kernels sit under
(/root/reference/tzrec/modules/embedding.py:993-1498): one torchrec ``EmbeddingCollection`` per
embedding dim (:1193-1197) returning a ``JaggedTensor`` per key, ``to_padded_dense(max_len)``
(:1429,1480), and the DIN target-attention encoder on the padded sequence
(/root/reference/tzrec/modules/sequence.py:65-128).

Kernels: the unpooled lookup is ``tzr_rows_gather`` (one row per id); its backward hands per-id
gradient rows to the same sort + fused-optimizer kernels as the pooled path (``grad_mode`` 1), so
duplicate ids inside and across sequences are summed exactly once per row; padding is
``tzr_jagged_to_padded_dense`` / ``tzr_padded_dense_to_jagged``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib
from .dlrm import MLP
from .embedding import EmbeddingBagCollection, EmbeddingBagConfig, SparseOptimizerConfig
from .sparse_bwd import SparseBackward, grad_dsts
from .sparse import JaggedTensor, KeyedJaggedTensor  # noqa: F401  (JaggedTensor re-exported)


@dataclass
class EmbeddingConfig:
    """torchrec EmbeddingConfig fields tzrec fills (tzrec/features/feature.py:638-662)."""

    name: str
    embedding_dim: int
    num_embeddings: int
    feature_names: List[str] = field(default_factory=list)
    init_fn: Optional[object] = None


class _J2PFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, offsets, max_len, pad):
        values = values.contiguous()
        B, D = offsets.numel() - 1, values.shape[1]
        out = torch.empty(B, max_len, D, dtype=torch.float32, device=values.device)
        rc = _lib.lib().tzr_jagged_to_padded_dense(_lib.ptr(values), values.stride(0), _lib.ptr(offsets), B,
                                                   max_len, D, float(pad), _lib.ptr(out), _lib.stream_ptr(values.device))
        _lib.check(rc, "tzr_jagged_to_padded_dense")
        ctx.save_for_backward(offsets)
        ctx.shape = (values.shape[0], D, max_len)
        return out

    @staticmethod
    def backward(ctx, g):
        (offsets,) = ctx.saved_tensors
        N, D, max_len = ctx.shape
        g = g.contiguous()
        gv = torch.empty(max(N, 1), D, dtype=torch.float32, device=g.device)
        rc = _lib.lib().tzr_padded_dense_to_jagged(_lib.ptr(g), _lib.ptr(offsets), offsets.numel() - 1, max_len, D,
                                                   _lib.ptr(gv), gv.stride(0), _lib.stream_ptr(g.device))
        _lib.check(rc, "tzr_padded_dense_to_jagged")
        return gv[:N], None, None, None


def jagged_to_padded_dense(values: torch.Tensor, offsets: torch.Tensor, max_len: int, padding_value: float = 0.0) -> torch.Tensor:
    """[N, D] + offsets[B+1] -> [B, max_len, D] (K12)."""
    return _J2PFn.apply(values, offsets, int(max_len), float(padding_value))


class _SegmentReduceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, offsets, mode):
        values = values.contiguous()
        S, D = offsets.numel() - 1, values.shape[1]
        out = torch.empty(max(S, 1), D, dtype=torch.float32, device=values.device)
        _lib.check(_lib.lib().tzr_segment_reduce_fwd(_lib.ptr(values), values.stride(0), _lib.ptr(offsets), S, D, mode,
                                                     _lib.ptr(out), out.stride(0), _lib.stream_ptr(values.device)),
                   "tzr_segment_reduce_fwd")
        ctx.save_for_backward(offsets)
        ctx.cfg = (values.shape[0], D, mode)
        return out[:S]

    @staticmethod
    def backward(ctx, g):
        (offsets,) = ctx.saved_tensors
        N, D, mode = ctx.cfg
        g = g.contiguous()
        gv = torch.empty(max(N, 1), D, dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().tzr_segment_reduce_bwd(_lib.ptr(g), g.stride(0) if g.numel() else D, _lib.ptr(offsets),
                                                     offsets.numel() - 1, D, mode, _lib.ptr(gv), gv.stride(0),
                                                     _lib.stream_ptr(g.device)), "tzr_segment_reduce_bwd")
        return gv[:N], None, None


def segment_reduce(values: torch.Tensor, lengths: torch.Tensor, pooling: str = "sum") -> torch.Tensor:
    """[N, D] rows + segment lengths [S] (sum = N) -> [S, D]: the rows of one multi-valued sequence
    step pooled into the step's row (`torch.segment_reduce(values, pooling, lengths=...)` followed by
    `nan_to_num` for the mean of an empty step, tzrec/modules/embedding.py:1353-1366)."""
    if pooling not in ("sum", "mean"):
        raise ValueError(f"segment_reduce pooling {pooling!r}: sum | mean")
    off = torch.zeros(lengths.numel() + 1, dtype=torch.int64, device=values.device)
    torch.cumsum(lengths.to(torch.int64), 0, out=off[1:])
    return _SegmentReduceFn.apply(values, off, 1 if pooling == "mean" else 0)


class _UnpooledLookupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ec, kjt, hook):
        out = ec._launch_forward(kjt)
        ctx.ec, ctx.kjt = ec, kjt
        return out

    @staticmethod
    def backward(ctx, g):
        ctx.ec._launch_backward(ctx.kjt, g)
        return None, None, None


class EmbeddingCollection(nn.Module):
    """Unpooled lookup: ``forward(KJT) -> {key: JaggedTensor}`` (one embedding row per id).  All
    tables of one collection share ``embedding_dim`` (the reference builds one EC per dim)."""

    def __init__(self, tables: Sequence[EmbeddingConfig], device=None, optimizer: Optional[SparseOptimizerConfig] = None,
                 row_layout: str = "interleaved") -> None:
        super().__init__()
        dims = {t.embedding_dim for t in tables}
        if len(dims) != 1:
            raise ValueError("one EmbeddingCollection per embedding_dim")
        self.dim = dims.pop()
        self._device = torch.device(device) if device is not None else torch.device("cpu")
        self._opt_cfg = optimizer
        # storage, init and optimizer state are the pooled module's
        self._store = EmbeddingBagCollection(
            [EmbeddingBagConfig(t.name, t.embedding_dim, t.num_embeddings, list(t.feature_names), "sum", t.init_fn) for t in tables],
            device=self._device, optimizer=optimizer, row_layout=row_layout)
        self.fused_optimizer = self._store.fused_optimizer
        self._meta_cache: Dict[tuple, dict] = {}
        self._hook = torch.zeros(0, requires_grad=True, device=self._device)
        self._lookup_trackers: list = []

    def register_post_lookup_tracker_fn(self, fn) -> None:
        """See EmbeddingBagCollection.register_post_lookup_tracker_fn."""
        self._lookup_trackers.append(fn)

    def table_weights(self):
        return self._store.table_weights()

    def table_states(self):
        return self._store.table_states()

    def _meta(self, keys: Sequence[str]) -> dict:
        ck = tuple(keys)
        m = self._meta_cache.get(ck)
        if m is not None:
            return m
        st = self._store
        base = st._meta([lk.key for lk in st._lookups], st._default_layout()) if all(
            lk.key in keys for lk in st._lookups) else None
        if base is None:
            raise KeyError("KeyedJaggedTensor lacks a key served by this EmbeddingCollection")
        table_of = {lk.key: lk.table for lk in st._lookups}
        K = len(keys)
        kt = np.array([table_of.get(k, -1) for k in keys], dtype=np.int32)
        if (kt < 0).any():
            raise KeyError("EmbeddingCollection expects a KJT holding exactly the keys it serves")
        tables = base.tables_np.copy()
        feats = np.zeros(K, dtype=_lib.FEATURE_DT)
        feats["dst"] = -1
        order = np.lexsort((np.arange(K), kt))
        rank_of = np.empty(K, dtype=np.int32)
        rank_of[order] = np.arange(K, dtype=np.int32)
        feats["table"], feats["key"], feats["order"] = kt, np.arange(K, dtype=np.int32), rank_of
        for t in range(len(tables)):
            mine = np.nonzero(kt == t)[0]
            tables[t]["first_order"] = int(rank_of[mine].min()) if len(mine) else 0
            tables[t]["n_feats"] = len(mine)
        m = {"d_tables": _lib.upload_struct(tables, self._device), "d_feats": _lib.upload_struct(feats, self._device),
             "d_key_table": torch.from_numpy(kt).to(self._device), "K": K, "T": len(tables),
             "max_rows": int(max(c.num_embeddings for c in st._configs))}
        self._meta_cache[ck] = m
        return m

    def _key_start(self, kjt: KeyedJaggedTensor) -> torch.Tensor:
        return kjt.offsets()[:: kjt.stride()].contiguous()  # [K+1] start of every key segment

    def _launch_forward(self, kjt: KeyedJaggedTensor) -> torch.Tensor:
        m = self._meta(kjt.keys())
        N = kjt.values().numel()
        out = torch.empty(max(N, 1), self.dim, dtype=torch.float32, device=self._device)
        ks = self._key_start(kjt)
        kjt._tzr_key_start = ks  # type: ignore[attr-defined]
        rc = _lib.lib().tzr_rows_gather(_lib.ptr(m["d_tables"]), _lib.ptr(m["d_key_table"]), _lib.ptr(ks), m["K"],
                                        _lib.ptr(kjt.values()), N, _lib.ptr(out), self.dim, self.dim,
                                        _lib.stream_ptr(self._device))
        _lib.check(rc, "tzr_rows_gather")
        return out[:N]

    def _launch_backward(self, kjt: KeyedJaggedTensor, g: torch.Tensor) -> None:
        if self.fused_optimizer is None:
            return
        m = self._meta(kjt.keys())
        N = kjt.values().numel()
        if N == 0:
            return
        g = g.contiguous().float()
        dev = self._device
        # one gradient row per id; the ids of key k lie behind key_start[k]
        p = SparseBackward(dev, m["d_tables"], m["d_feats"], m["T"], m["K"], m["K"], m["max_rows"], self.dim, kjt.values(),
                           kjt._tzr_key_start, None, N, N, 1, grad_mode=1)  # type: ignore[attr-defined]
        ws = _lib.workspace(p.plan_bytes(), dev)
        p.plan(ws)
        self.fused_optimizer.begin_step(dev)
        p.apply(ws, grad_dsts([g]), self.fused_optimizer.optim_struct(dev))

    def forward(self, features: KeyedJaggedTensor) -> Dict[str, JaggedTensor]:
        if self._lookup_trackers:
            table_of = {f: c.name for c in self._store.embedding_bag_configs() for f in c.feature_names}
            segs = tuple((table_of[k], i) for i, k in enumerate(features.keys()))
            for fn in self._lookup_trackers:
                fn(self, segs, features.values(), features.offsets(), features.stride(), 0)
        if torch.is_grad_enabled() and self.fused_optimizer is not None and self.training:
            rows = _UnpooledLookupFn.apply(self, features, self._hook)
        else:
            rows = self._launch_forward(features)
        B = features.stride()
        off, lens = features.offsets(), features.lengths()
        lpk = features.length_per_key()
        # (one split, not a slice per key: the backward of a slice is a zero tensor of ALL rows plus an add into the sum of
        # the others -- eight 90 MB fills and adds per multi_tower_din step; the backward of a split is one concatenation)
        segs = torch.split(rows, [int(n) for n in lpk], dim=0)
        out = {}
        for i, k in enumerate(features.keys()):
            o = off[i * B:(i + 1) * B + 1] - off[i * B]
            out[k] = JaggedTensor(segs[i], lens[i * B:(i + 1) * B], o)
        return out


class _ShardedUnpooledFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ec, kjt, hook):
        rows, st = ec._forward_impl(kjt)
        ctx.ec, ctx.st = ec, st
        return rows

    @staticmethod
    def backward(ctx, g):
        ctx.ec._backward_impl(ctx.st, g)
        return None, None, None


class ShardedEmbeddingCollection(nn.Module):
    """Unpooled lookup over tables sharded across ranks (BASELINE config 4 on 8 GPUs: the sequence
    features of multi_tower_din).  It is the id-granularity exchange of `sharding.py` with the last
    step left out: the rows come back from their owners one per id, and instead of pooling them the
    requester just puts them back in lookup order; backward sends one gradient row per id to the
    owner, whose sort + fused update is the per-id mode it already runs for pooled tables.

    `forward(KJT) -> {key: JaggedTensor}` in the collection's key order (table, then feature).  All
    tables take part in the exchange (row-wise by default, `constraints` for table-wise)."""

    def __init__(self, tables: Sequence[EmbeddingConfig], device, optimizer: Optional[SparseOptimizerConfig] = None,
                 process_group=None, constraints: Optional[Dict[str, str]] = None) -> None:
        super().__init__()
        from .sharding import ShardedEmbeddingBagCollection

        self.sharded = ShardedEmbeddingBagCollection(
            [EmbeddingBagConfig(t.name, t.embedding_dim, t.num_embeddings, list(t.feature_names), "sum", t.init_fn) for t in tables],
            device=device, optimizer=optimizer, process_group=process_group, dp_max_rows=0, constraints=constraints)
        self.dim = self.sharded.dim
        self._device = torch.device(device)
        self.fused_optimizer = self.sharded.fused_optimizer
        self._hook = torch.zeros(0, requires_grad=True, device=self._device)

    def table_weights(self):
        return self.sharded.table_weights()

    def _forward_impl(self, kjt: KeyedJaggedTensor):
        sh = self.sharded
        st = sh.input_dist_end(sh.input_dist_begin(kjt, ("__all__",)))
        rows_in, _, work = sh.exchange_rows(st)
        work.wait()
        N = st["N_rw"]
        rows = rows_in[:N].index_select(0, st["unb"]) if N else rows_in[:0]  # bucketized order -> lookup order
        return rows, st

    def _backward_impl(self, st: dict, g: torch.Tensor) -> None:
        N = st["N_rw"]
        grow = torch.empty(max(N, 1), self.dim, dtype=torch.float32, device=self._device)
        if N:
            grow[:N].index_copy_(0, st["unb"], g.contiguous().float())  # lookup order -> bucketized order
        self.sharded._backward_impl(st, [], id_grads=grow)

    def forward(self, features: KeyedJaggedTensor) -> Dict[str, JaggedTensor]:
        if torch.is_grad_enabled() and self.fused_optimizer is not None and self.training:
            rows = _ShardedUnpooledFn.apply(self, features, self._hook)
            st_sub = None
        else:
            rows, _ = self._forward_impl(features)
        sh = self.sharded
        rm = sh._requester_meta(features.keys(), sh._layout_for(("__all__",)))
        perm = rm["rw_perm"]
        sub = features if perm == list(range(len(features.keys()))) else features.permute(perm)
        B = sub.stride()
        off, lens, lpk = sub.offsets(), sub.lengths(), sub.length_per_key()
        out, start = {}, 0
        for i, k in enumerate(sub.keys()):
            o = off[i * B:(i + 1) * B + 1] - off[i * B]
            out[k] = JaggedTensor(rows[start:start + lpk[i]], lens[i * B:(i + 1) * B], o)
            start += lpk[i]
        return out


# ---- DIN target attention on the jagged positions (csrc/din_attention.hip) -------------------------------------------
def jagged_segment_ids(offsets: torch.Tensor, n: int) -> torch.Tensor:
    """sample of every row of a jagged [n, .] tensor (int32 [n]); rows at or behind offsets[-1] get B"""
    seg = torch.empty(max(n, 1), dtype=torch.int32, device=offsets.device)
    _lib.check(_lib.lib().tzr_jagged_segment_ids(_lib.ptr(offsets), offsets.numel() - 1, n, _lib.ptr(seg), _lib.stream_ptr(offsets.device)),
               "tzr_jagged_segment_ids")
    return seg[:n]


class _DinTowerFn(torch.autograd.Function):
    """The whole DIN tower on the jagged positions as ONE autograd node:

        X = [k | q * k | q]  (tzr_din_assemble_fwd)  ->  relu(X W1'^T + b1) -> ... -> h  (one GEMM per layer, ReLU in its epilogue)
        -> s = h . w + b, softmax over every sample's rows, out_b = sum_n p_n k_n  (tzr_din_attn_fwd)

    and its backward spelled out: tzr_din_attn_bwd -> tzr_head_bwd (the one-unit score layer) -> per layer ReLU mask + bias
    gradient in one pass (tzr_relu_bwd_colsum), weight gradient as 16 batched products + sum (dense.weight_grad), input
    gradient -> tzr_din_assemble_bwd, which ADDS the attention's direct part of the rows' gradient.  One node instead of a
    graph of them: no gradient-accumulation adds, no zero fills, no contiguous copies between the pieces.  `wb` = (W1, b1, W2, b2, ...) with W1 the
    reference's [H, 4 D] first layer: folded to three blocks here, its gradient unfolded."""

    @staticmethod
    def forward(ctx, values, query, offsets, max_len, row_bucket, w3, b3, *wb):
        values, query = values.contiguous(), query.contiguous()
        N, D = values.shape
        B = offsets.numel() - 1
        dev = values.device
        L = _lib.lib()
        stream = _lib.stream_ptr(dev)
        if _DinTowerFn._own_products(values, query, wb):
            return _DinTowerFn._forward_own(ctx, values, query, offsets, max_len, w3, b3, wb)
        ctx.own = False
        Np = (N + row_bucket - 1) // row_bucket * row_bucket
        seg = jagged_segment_ids(offsets, Np)
        X = torch.empty(max(Np, 1), 3 * D, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_assemble_fwd(_lib.ptr(values), values.stride(0), _lib.ptr(query), query.stride(0), _lib.ptr(seg), B, Np, D,
                                          _lib.ptr(X), X.stride(0), stream), "tzr_din_assemble_fwd")
        Ws = [w.detach() for w in wb[0::2]]
        bs = [b_.detach() for b_ in wb[1::2]]
        W1 = Ws[0]
        Ws[0] = torch.cat([W1[:, D:2 * D] - W1[:, 2 * D:3 * D], W1[:, 3 * D:], W1[:, :D] + W1[:, 2 * D:3 * D]], dim=1)
        x, hs = X[:Np], []
        for w, b_ in zip(Ws, bs):
            x = torch._addmm_activation(b_, x, w.t(), use_gelu=False) if x.is_cuda else torch.relu(torch.nn.functional.linear(x, w, b_))
            hs.append(x)
        H = x.shape[1]
        w3v = w3.detach().reshape(-1).contiguous()
        out = torch.empty(max(B, 1), D, dtype=torch.float32, device=dev)
        p = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_attn_fwd(_lib.ptr(x), x.stride(0) if Np else H, H, _lib.ptr(w3v), _lib.ptr(b3), _lib.ptr(values),
                                      values.stride(0) if N else D, D, _lib.ptr(offsets), B, max_len, _lib.ptr(out), out.stride(0),
                                      _lib.ptr(p), stream), "tzr_din_attn_fwd")
        ctx.save_for_backward(values, query, offsets, seg, p, w3, X, *Ws, *hs)
        ctx.cfg = (max_len, len(Ws), b3 is not None)
        return out[:B]

    # ---- the same tower with its products on the library's own tall-input kernels (csrc/gemm_rows.hip) and the query's block of
    # the first layer taken once per SAMPLE: W1 [q, k, q - k, q * k] = (Wb - Wc) k + Wd (q * k) + [(Wa + Wc) q + b1], the bracket a
    # [B, H1] product whose rows the per-position kernel gathers.  No row bucket (no library to key by shape), no GEMM library call.
    @staticmethod
    def _own_products(values, query, wb) -> bool:
        from . import dense
        from .dense import linear_rows_supported, linear_rows_wgrad_supported

        N, D = values.shape
        if N < dense.ROWS_GEMM_MIN_ROWS and values.is_cuda or N == 0 or query.shape[0] == 0 or len(wb) < 4 or any(t is None for t in wb):
            return False  # (few rows: the library's small tiles do as well; a layer without bias: the library path)
        L = _lib.lib()
        Hs = [w.shape[0] for w in wb[0::2]]
        Ks = [2 * D] + Hs[:-1]
        if wb[0].shape[1] != 4 * D or not L.tzr_linear_rows_supported(D, Hs[0]) or not L.tzr_linear_rows_supported(Hs[0], D) \
                or not L.tzr_linear_rows_wgrad_supported(Hs[0], D):
            return False
        for i, (K, H) in enumerate(zip(Ks, Hs)):
            if not (L.tzr_linear_rows_supported(K, H) and L.tzr_linear_rows_wgrad_supported(H, K)):
                return False
            if i == 0 and not (L.tzr_linear_rows_supported(K, H) & 2 and L.tzr_linear_rows_supported(H, K)):  # row-vector form; its input gradient
                return False
            if i > 0 and not L.tzr_linear_bwd_relu_supported(H, K):
                return False
        return linear_rows_supported(values, D, Hs[0]) and values.dtype == torch.float32 and all(w.dtype == torch.float32 for w in wb)

    own_calls = 0  # forwards that took the library's own products (tests)

    @staticmethod
    def _forward_own(ctx, values, query, offsets, max_len, w3, b3, wb):
        from .dense import linear_rows

        _DinTowerFn.own_calls += 1

        N, D = values.shape
        B = offsets.numel() - 1
        dev = values.device
        L = _lib.lib()
        stream = _lib.stream_ptr(dev)
        seg = jagged_segment_ids(offsets, N)
        X = torch.empty(N, 2 * D, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_assemble2_fwd(_lib.ptr(values), values.stride(0), _lib.ptr(query), query.stride(0), _lib.ptr(seg), B, N, D,
                                           _lib.ptr(X), X.stride(0), stream), "tzr_din_assemble2_fwd")
        Ws = [w.detach() for w in wb[0::2]]
        bs = [b_.detach() for b_ in wb[1::2]]
        W1 = Ws[0]
        Wq = (W1[:, :D] + W1[:, 2 * D:3 * D]).contiguous()                                  # [H1, D]
        Ws[0] = torch.cat([W1[:, D:2 * D] - W1[:, 2 * D:3 * D], W1[:, 3 * D:]], dim=1)      # [H1, 2 D]
        hq = linear_rows(query, Wq, bs[0])                                                   # [B, H1]: (Wa + Wc) q + b1
        x, hs = X, []
        for i, (w, b_) in enumerate(zip(Ws, bs)):
            x = linear_rows(x, w, None, relu=True, rowvec=hq, row_index=seg) if i == 0 else linear_rows(x, w, b_, relu=True)
            hs.append(x)
        H = x.shape[1]
        w3v = w3.detach().reshape(-1).contiguous()
        out = torch.empty(max(B, 1), D, dtype=torch.float32, device=dev)
        p = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_attn_fwd(_lib.ptr(x), x.stride(0), H, _lib.ptr(w3v), _lib.ptr(b3), _lib.ptr(values), values.stride(0), D,
                                      _lib.ptr(offsets), B, max_len, _lib.ptr(out), out.stride(0), _lib.ptr(p), stream), "tzr_din_attn_fwd")
        ctx.save_for_backward(values, query, offsets, seg, p, w3, X, Wq, *Ws, *hs)
        ctx.cfg = (max_len, len(Ws), b3 is not None)
        ctx.own = True
        return out[:B]

    @staticmethod
    def _backward_own(ctx, gout):
        from .dense import head_bwd_relu, linear_bwd_relu, linear_rows, linear_rows_wgrad

        max_len, nl, has_b3 = ctx.cfg
        values, query, offsets, seg, p, w3, X, Wq = ctx.saved_tensors[:8]
        Ws, hs = ctx.saved_tensors[8:8 + nl], ctx.saved_tensors[8 + nl:]
        N, D = values.shape
        B = offsets.numel() - 1
        dev = values.device
        L = _lib.lib()
        stream = _lib.stream_ptr(dev)
        gout = gout.contiguous()
        ds = torch.empty(N, dtype=torch.float32, device=dev)
        dkv = torch.empty(N, D, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_attn_bwd(_lib.ptr(gout), gout.stride(0), _lib.ptr(p), _lib.ptr(values), values.stride(0), D, _lib.ptr(offsets), B,
                                      max_len, _lib.ptr(ds), _lib.ptr(dkv), dkv.stride(0), stream), "tzr_din_attn_bwd")
        g, dw3, db3, gb = head_bwd_relu(ds, hs[-1], w3)
        grads_wb = [None] * (2 * nl)
        for i in range(nl - 1, 0, -1):  # g = the gradient at layer i's pre-activation, gb = its column sums
            grads_wb[2 * i] = linear_rows_wgrad(g, hs[i - 1])
            grads_wb[2 * i + 1] = gb
            g, gb = linear_bwd_relu(g, Ws[i], hs[i - 1])
        # first layer: its per-position block [Wb - Wc | Wd] and, through the per-sample sums of g, the query's block Wa + Wc
        dWk = linear_rows_wgrad(g, X)                                   # [H1, 2 D]
        dX = linear_rows(g, Ws[0], out_major=False)                     # [N, 2 D]
        H1 = g.shape[1]
        dhq = torch.empty(max(B, 1), H1, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_segment_reduce_fwd(_lib.ptr(g), g.stride(0), _lib.ptr(offsets), B, H1, 0, _lib.ptr(dhq), dhq.stride(0), stream),
                   "tzr_segment_reduce_fwd")
        dhq = dhq[:B]
        dWq = linear_rows_wgrad(dhq, query)                             # [H1, D]
        dq_add = linear_rows(dhq, Wq, out_major=False)                  # [B, D]
        grads_wb[0] = torch.cat([dWq, dWk[:, :D], dWq - dWk[:, :D], dWk[:, D:]], dim=1)  # [dWa | dWb | dWc | dWd]
        grads_wb[1] = gb
        dq = torch.empty(max(B, 1), D, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_assemble2_bwd(_lib.ptr(dX), dX.stride(0), _lib.ptr(values), values.stride(0), _lib.ptr(query), query.stride(0),
                                           _lib.ptr(seg), _lib.ptr(offsets), B, N, D, _lib.ptr(dkv), dkv.stride(0), 1, _lib.ptr(dq_add),
                                           dq_add.stride(0), _lib.ptr(dq), dq.stride(0), stream), "tzr_din_assemble2_bwd")
        return (dkv, dq[:B], None, None, None, dw3.reshape(w3.shape), (db3 if has_b3 else None), *grads_wb)

    @staticmethod
    def backward(ctx, gout):
        from .dense import head_bwd_relu, linear_bwd_relu, linear_bwd_relu_supported, relu_bwd_colsum, weight_grad

        if ctx.own:
            return _DinTowerFn._backward_own(ctx, gout)
        max_len, nl, has_b3 = ctx.cfg
        values, query, offsets, seg, p, w3, X = ctx.saved_tensors[:7]
        Ws, hs = ctx.saved_tensors[7:7 + nl], ctx.saved_tensors[7 + nl:]
        N, D = values.shape
        B, Np = offsets.numel() - 1, seg.numel()
        dev = values.device
        L = _lib.lib()
        stream = _lib.stream_ptr(dev)
        gout = gout.contiguous()
        ds = torch.empty(max(Np, 1), dtype=torch.float32, device=dev) if Np == N else torch.zeros(Np, dtype=torch.float32, device=dev)
        dkv = torch.empty(max(Np, 1), D, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_attn_bwd(_lib.ptr(gout), gout.stride(0) if B else D, _lib.ptr(p), _lib.ptr(values), values.stride(0) if N else D, D,
                                      _lib.ptr(offsets), B, max_len, _lib.ptr(ds), _lib.ptr(dkv), dkv.stride(0), stream), "tzr_din_attn_bwd")
        h = hs[-1]
        H = h.shape[1]
        kernels = bool(Np) and all(y.shape[1] % 4 == 0 and y.shape[1] <= 1024 for y in hs)
        # the score layer's backward chained with the last hidden layer's mask + bias gradient (tzr_head_bwd_relu)
        if kernels:
            g, dw3, db3, gb = head_bwd_relu(ds[:Np], h, w3)
        else:
            dsn = ds[:Np]
            dh, dw3, db3 = dsn.unsqueeze(1) * w3.reshape(1, -1), (h * dsn.unsqueeze(1)).sum(0, keepdim=True), dsn.sum().reshape(1)
            g = torch.ops.aten.threshold_backward(dh, h, 0.0)
            gb = g.sum(0)
        grads_wb = [None] * (2 * nl)
        for i in range(nl - 1, -1, -1):  # g = the gradient at layer i's pre-activation, gb = its column sums
            xin = hs[i - 1] if i > 0 else X[:Np]
            grads_wb[2 * i] = weight_grad(g, xin) if Np else torch.zeros_like(Ws[i])
            grads_wb[2 * i + 1] = gb
            if i == 0:
                dh = g @ Ws[0]
            elif kernels and linear_bwd_relu_supported(g, Ws[i]):
                g, gb = linear_bwd_relu(g, Ws[i], hs[i - 1])  # (g W_i) masked by layer i - 1's ReLU + its column sums: d(loss)/d(h) never written
            elif kernels:
                g, gb = relu_bwd_colsum(g @ Ws[i], hs[i - 1])
            else:
                g = torch.ops.aten.threshold_backward(g @ Ws[i], hs[i - 1], 0.0)
                gb = g.sum(0)
        dWf = grads_wb[0]  # [H1, 3 D] = [d(Wb - Wc) | dWd | d(Wa + Wc)]  ->  [dWa | dWb | dWc | dWd]
        grads_wb[0] = torch.cat([dWf[:, 2 * D:], dWf[:, :D], dWf[:, 2 * D:] - dWf[:, :D], dWf[:, D:2 * D]], dim=1)
        dX = dh.contiguous()
        dq = torch.empty(max(B, 1), D, dtype=torch.float32, device=dev)
        _lib.check(L.tzr_din_assemble_bwd(_lib.ptr(dX), dX.stride(0) if Np else 3 * D, _lib.ptr(values), values.stride(0), _lib.ptr(query),
                                          query.stride(0), _lib.ptr(seg), _lib.ptr(offsets), B, Np, D, _lib.ptr(dkv), dkv.stride(0), 1,
                                          _lib.ptr(dq), dq.stride(0), stream), "tzr_din_assemble_bwd")
        return (dkv[:N], dq[:B], None, None, None, dw3.reshape(w3.shape), (db3 if has_b3 else None), *grads_wb)


DIN_JAGGED_MAX_LEN = 2048  # (DA_MAXLEN of csrc/din_attention.hip: scores of one sample kept in LDS)
DIN_JAGGED_MAX_DIM = 256  # (tzr_din_assemble_bwd: one wave holds a row of the query gradient, 4 * TZR_WAVE floats)


class DINEncoder(nn.Module):
    """DIN target attention (same constructor/forward contract as the reference's DINEncoder,
    tzrec/modules/sequence.py:65-128): scores = MLP([q, k, q-k, q*k]) -> masked softmax -> sum.

    Two evaluations of the same function: on the PADDED `<input>.sequence` [B, L, D] (the reference's tensors), or -- when the
    embedding group hands over `<input>.sequence_jagged` ([N, D] rows of the unpooled lookup) and `<input>.sequence_offsets`
    -- on the jagged positions (`forward_jagged`): no padding position is ever computed (csrc/din_attention.hip)."""

    def __init__(self, sequence_dim: int, query_dim: int, input: str, attn_mlp: Dict[str, object], max_seq_length: int = 0) -> None:
        super().__init__()
        if query_dim > sequence_dim:
            raise ValueError("query_dim > sequence_dim not supported yet.")
        self._input = input
        self._query_dim, self._sequence_dim, self._max_seq_length = query_dim, sequence_dim, max_seq_length
        self.mlp = MLP(sequence_dim * 4, list(attn_mlp["hidden_units"]))
        self.linear = nn.Linear(self.mlp.hidden_units[-1], 1)
        self._query_name = f"{input}.query"
        self._sequence_name = f"{input}.sequence"
        self._sequence_length_name = f"{input}.sequence_length"
        self.split_first_layer = True  # see forward; False = the reference's literal [q, k, q - k, q * k] input
        self.row_bucket = None  # forward_jagged: rows of the attention MLP's input = N rounded up to a multiple of this (None: 16384 on a GPU, 1 elsewhere)

    def input(self) -> str:
        return self._input

    def output_dim(self) -> int:
        return self._sequence_dim

    def jagged_limit(self) -> Optional[str]:
        """None when `forward_jagged` evaluates this encoder, else the limit of csrc/din_attention.hip it is outside of"""
        D, H = self._sequence_dim, self.mlp.hidden_units[-1]
        if not getattr(self.mlp, "_plain", False):
            return "the attention MLP must be plain Linear + bias + ReLU layers"
        if D % 4:
            return f"sequence_dim {D} must be a multiple of 4"
        if D > DIN_JAGGED_MAX_DIM:
            return f"sequence_dim {D} must be at most {DIN_JAGGED_MAX_DIM}"
        if H % 4:
            return f"the last attention-MLP width {H} must be a multiple of 4"
        return None

    def jagged_capable(self) -> bool:
        """plain Linear + bias + ReLU layers (the reference's defaults) within the kernels' limits: what `forward_jagged` evaluates"""
        return self.jagged_limit() is None

    def _folded_first_layer(self) -> torch.Tensor:
        """W [q, k, q - k, q * k] = (Wb - Wc) k + Wd (q * k) + (Wa + Wc) q  ->  [Wb - Wc | Wd | Wa + Wc]  ([H, 3 D])"""
        D = self._sequence_dim
        W = self.mlp.mlp[0].weight
        return torch.cat([W[:, D:2 * D] - W[:, 2 * D:3 * D], W[:, 3 * D:], W[:, :D] + W[:, 2 * D:3 * D]], dim=1)

    def forward_jagged(self, query: torch.Tensor, values: torch.Tensor, offsets: torch.Tensor, max_len: int) -> torch.Tensor:
        """query [B, query_dim]; values [N, D]: the rows of all samples' sequences, sample b = rows [offsets[b], offsets[b+1]);
        max_len: positions at index >= max_len inside a sample do not take part (the padded length of the reference's
        `sequence` tensor; `max_seq_length` is applied on top).  Same output and gradients as `forward` on the padded form."""

        limit = self.jagged_limit()
        if limit is not None:
            raise ValueError(f"DINEncoder.forward_jagged: {limit} (use the padded form)")
        if self._max_seq_length > 0:
            max_len = min(max_len, self._max_seq_length)
        if max_len > DIN_JAGGED_MAX_LEN:
            raise ValueError(f"DINEncoder.forward_jagged: max_len {max_len} must be at most {DIN_JAGGED_MAX_LEN} (use the padded form)")
        if self._query_dim < self._sequence_dim:
            query = nn.functional.pad(query, (0, self._sequence_dim - self._query_dim))
        # the attention MLP runs on Np >= N rows, N rounded up to `row_bucket`: a GEMM library tunes (and TunableOp keys) its
        # kernels by exact shape, and every batch has its own N -- with buckets a handful of shapes serve them all; the
        # rows behind N are zero inputs whose outputs nothing reads and whose gradients are zero
        rb = max(int(self.row_bucket), 1) if self.row_bucket is not None else (16384 if values.is_cuda else 1)
        wb = []
        for m in self.mlp.linears():
            wb += [m.weight, m.bias]
        return _DinTowerFn.apply(values, query, offsets, int(max_len), rb, self.linear.weight, self.linear.bias, *wb)

    def forward(self, sequence_embedded: Dict[str, torch.Tensor]) -> torch.Tensor:
        jag = sequence_embedded.get(self._sequence_name + "_jagged")
        if jag is not None:
            return self.forward_jagged(sequence_embedded[self._query_name], jag, sequence_embedded[self._sequence_name + "_offsets"],
                                       int(sequence_embedded[self._sequence_name + "_max_len"]))
        query = sequence_embedded[self._query_name]
        sequence = sequence_embedded[self._sequence_name]
        sequence_length = sequence_embedded[self._sequence_length_name]
        if self._max_seq_length > 0:
            sequence_length = torch.clamp_max(sequence_length, self._max_seq_length)
            sequence = sequence[:, : self._max_seq_length, :]
        L = sequence.size(1)
        mask = torch.arange(L, device=sequence_length.device).unsqueeze(0) < sequence_length.unsqueeze(1)
        if self._query_dim < self._sequence_dim:
            query = nn.functional.pad(query, (0, self._sequence_dim - self._query_dim))
        first = self.mlp.mlp[0]
        if self.split_first_layer and isinstance(first, nn.Linear):
            # W [q, k, q - k, q * k] = (Wa + Wc) q + (Wb - Wc) k + Wd (q * k): the query part is one row per SAMPLE, not per
            # position, the per-position product has half the contraction length (k and q * k), and the [B, L, 4 D] input
            # (420 MB at B = 8 192, L = 100, D = 32) is never built.  Same sums reassociated: ~1e-7 relative.
            D = self._sequence_dim
            W = first.weight
            wq = W[:, :D] + W[:, 2 * D:3 * D]
            wk = torch.cat([W[:, D:2 * D] - W[:, 2 * D:3 * D], W[:, 3 * D:]], dim=1)
            hq = nn.functional.linear(query, wq, first.bias)  # [B, H]
            h = nn.functional.linear(torch.cat([sequence, query.unsqueeze(1) * sequence], dim=-1), wk) + hq.unsqueeze(1)
            a = self.linear(self.mlp.mlp[1:](h)).transpose(1, 2)
        else:
            q = query.unsqueeze(1).expand(-1, L, -1)
            a = self.linear(self.mlp(torch.cat([q, sequence, q - sequence, q * sequence], dim=-1))).transpose(1, 2)
        scores = torch.where(mask.unsqueeze(1), a, torch.ones_like(a) * (-(2 ** 31) + 1))
        return torch.matmul(torch.softmax(scores, dim=-1), sequence).squeeze(1)


# ---- simple attention and pooling on the jagged positions (csrc/jagged_encoders.hip) ---------------------------------
JAGGED_ENCODER_MAX_LEN = 2048  # (JE_MAXLEN: tzr_jagged_dot_attn_* keep a sample's scores in LDS)
JAGGED_ENCODER_MAX_DIM = 256  # (JE_MAXDIM: one lane per float4 piece of a row)


class _JaggedDotAttnFn(torch.autograd.Function):
    """out_b = sum_n softmax_n(k_n . q_b) k_n over sample b's rows, one node: tzr_jagged_dot_attn_fwd / _bwd"""

    @staticmethod
    def forward(ctx, values, query, offsets, max_len):
        values, query = _lib.rows16(values), _lib.rows16(query)
        N, D = values.shape
        B = offsets.numel() - 1
        dev = values.device
        out = torch.empty(max(B, 1), D, dtype=torch.float32, device=dev)
        p = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().tzr_jagged_dot_attn_fwd(_lib.ptr(values), values.stride(0) if N else D, _lib.ptr(query),
                                                      query.stride(0) if B else D, D, _lib.ptr(offsets), B, N, max_len, _lib.ptr(out),
                                                      out.stride(0), _lib.ptr(p), _lib.stream_ptr(dev)), "tzr_jagged_dot_attn_fwd")
        ctx.save_for_backward(values, query, offsets, p)
        ctx.max_len = max_len
        return out[:B]

    @staticmethod
    def backward(ctx, gout):
        values, query, offsets, p = ctx.saved_tensors
        N, D = values.shape
        B = offsets.numel() - 1
        dev = values.device
        gout = _lib.rows16(gout)
        dkv = torch.empty(max(N, 1), D, dtype=torch.float32, device=dev)
        dq = torch.empty(max(B, 1), D, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().tzr_jagged_dot_attn_bwd(_lib.ptr(gout), gout.stride(0) if B else D, _lib.ptr(p), _lib.ptr(values),
                                                      values.stride(0) if N else D, _lib.ptr(query), query.stride(0) if B else D, D,
                                                      _lib.ptr(offsets), B, N, ctx.max_len, _lib.ptr(dkv), dkv.stride(0), _lib.ptr(dq),
                                                      dq.stride(0), _lib.stream_ptr(dev)), "tzr_jagged_dot_attn_bwd")
        return dkv[:N], dq[:B], None, None


class _JaggedPoolFn(torch.autograd.Function):
    """sum / mean of the first min(len, max_len) rows of every sample: tzr_jagged_pool_fwd / _bwd"""

    @staticmethod
    def forward(ctx, values, offsets, max_len, mode):
        values = _lib.rows16(values)
        N, D = values.shape
        B = offsets.numel() - 1
        out = torch.empty(max(B, 1), D, dtype=torch.float32, device=values.device)
        _lib.check(_lib.lib().tzr_jagged_pool_fwd(_lib.ptr(values), values.stride(0) if N else D, D, _lib.ptr(offsets), B, N, max_len, mode,
                                                  _lib.ptr(out), out.stride(0), _lib.stream_ptr(values.device)), "tzr_jagged_pool_fwd")
        ctx.save_for_backward(offsets)
        ctx.cfg = (N, D, max_len, mode)
        return out[:B]

    @staticmethod
    def backward(ctx, gout):
        (offsets,) = ctx.saved_tensors
        N, D, max_len, mode = ctx.cfg
        gout = _lib.rows16(gout)
        B = offsets.numel() - 1
        dkv = torch.empty(max(N, 1), D, dtype=torch.float32, device=gout.device)
        _lib.check(_lib.lib().tzr_jagged_pool_bwd(_lib.ptr(gout), gout.stride(0) if B else D, D, _lib.ptr(offsets), B, N, max_len, mode,
                                                  _lib.ptr(dkv), dkv.stride(0), _lib.stream_ptr(gout.device)), "tzr_jagged_pool_bwd")
        return dkv[:N], None, None, None


def jagged_dot_attention(values: torch.Tensor, query: torch.Tensor, offsets: torch.Tensor, max_len: int) -> torch.Tensor:
    """values [N, D] rows, query [B, D], offsets int64 [B + 1] -> [B, D]; positions at index >= max_len inside a sample do not
    take part; a sample without a position gives a zero row"""
    return _JaggedDotAttnFn.apply(values, query, offsets, int(max_len))


def jagged_pool(values: torch.Tensor, offsets: torch.Tensor, max_len: int, pooling: str = "mean") -> torch.Tensor:
    """values [N, D] rows, offsets int64 [B + 1] -> [B, D]: sum or mean (over max(count, 1)) of every sample's first
    min(len, max_len) rows"""
    if pooling not in ("sum", "mean"):
        raise ValueError(f"jagged_pool pooling {pooling!r}: sum | mean")
    return _JaggedPoolFn.apply(values, offsets, int(max_len), _lib.POOL_MEAN if pooling == "mean" else _lib.POOL_SUM)


def _jagged_dim_limit(what: str, D: int) -> Optional[str]:
    if D % 4:
        return f"{what}: sequence_dim {D} must be a multiple of 4"
    if D > JAGGED_ENCODER_MAX_DIM:
        return f"{what}: sequence_dim {D} must be at most {JAGGED_ENCODER_MAX_DIM}"
    return None


class SimpleAttention(nn.Module):
    """Dot-product attention of the query over the sequence (the reference's SimpleAttention, constructor and forward contract
    of tzrec/modules/sequence.py:131-171): scores = sequence . query -> masked softmax -> weighted sum.  Evaluated on the padded
    `<input>.sequence` [B, L, D] as the reference does, or -- when the dict carries `<input>.sequence_jagged`, `_offsets` and
    `_max_len` -- on the jagged rows (csrc/jagged_encoders.hip).  The reference multiplies [B, L, sequence_dim] by
    [B, query_dim, 1] and fails inside matmul when the two dims differ; here that is an error at construction."""

    def __init__(self, sequence_dim: int, query_dim: int, input: str, max_seq_length: int = 0, **kwargs) -> None:
        super().__init__()
        if query_dim != sequence_dim:
            raise ValueError(f"simple_attention on {input!r}: query_dim {query_dim} must equal sequence_dim {sequence_dim}")
        self._input = input
        self._sequence_dim, self._query_dim, self._max_seq_length = sequence_dim, query_dim, max_seq_length
        self._query_name = f"{input}.query"
        self._sequence_name = f"{input}.sequence"
        self._sequence_length_name = f"{input}.sequence_length"

    def input(self) -> str:
        return self._input

    def output_dim(self) -> int:
        return self._sequence_dim

    def jagged_limit(self, max_len: int = 0) -> Optional[str]:
        """None when the jagged kernels evaluate this encoder on sequences padded / truncated to `max_len`, else the limit missed"""
        lim = _jagged_dim_limit("simple_attention", self._sequence_dim)
        if lim is None and (min(max_len, self._max_seq_length) if self._max_seq_length > 0 else max_len) > JAGGED_ENCODER_MAX_LEN:
            lim = f"simple_attention: max_len {max_len} must be at most {JAGGED_ENCODER_MAX_LEN}"
        return lim

    def forward(self, sequence_embedded: Dict[str, torch.Tensor]) -> torch.Tensor:
        query = sequence_embedded[self._query_name]
        jag = sequence_embedded.get(self._sequence_name + "_jagged")
        if jag is not None:
            max_len = int(sequence_embedded[self._sequence_name + "_max_len"])
            limit = self.jagged_limit(max_len)
            if limit is not None:
                raise ValueError(f"{limit} (use the padded form)")
            if self._max_seq_length > 0:
                max_len = min(max_len, self._max_seq_length)
            return jagged_dot_attention(jag, query, sequence_embedded[self._sequence_name + "_offsets"], max_len)
        sequence = sequence_embedded[self._sequence_name]
        sequence_length = sequence_embedded[self._sequence_length_name]
        if self._max_seq_length > 0:
            sequence_length = torch.clamp_max(sequence_length, self._max_seq_length)
            sequence = sequence[:, : self._max_seq_length, :]
        mask = torch.arange(sequence.size(1), device=sequence_length.device).unsqueeze(0) < sequence_length.unsqueeze(1)
        a = torch.matmul(sequence, query.unsqueeze(2)).squeeze(2)
        scores = torch.softmax(torch.where(mask, a, torch.ones_like(a) * (-(2 ** 31) + 1)), dim=-1)
        return torch.matmul(scores.unsqueeze(1), sequence).squeeze(1)


class PoolingEncoder(nn.Module):
    """Sum / mean of the sequence (the reference's PoolingEncoder, tzrec/modules/sequence.py:174-218; the mean divides by
    max(length, 1)), on the padded `<input>.sequence` or on the jagged rows like `SimpleAttention`."""

    def __init__(self, sequence_dim: int, input: str, pooling_type: str = "mean", max_seq_length: int = 0, **kwargs) -> None:
        super().__init__()
        assert pooling_type in ["sum", "mean"], "only sum|mean pooling type supported now."
        self._input = input
        self._sequence_dim, self._pooling_type, self._max_seq_length = sequence_dim, pooling_type, max_seq_length
        self._sequence_name = f"{input}.sequence"
        self._sequence_length_name = f"{input}.sequence_length"

    def input(self) -> str:
        return self._input

    def output_dim(self) -> int:
        return self._sequence_dim

    def jagged_limit(self, max_len: int = 0) -> Optional[str]:
        return _jagged_dim_limit("pooling_encoder", self._sequence_dim)

    def forward(self, sequence_embedded: Dict[str, torch.Tensor]) -> torch.Tensor:
        jag = sequence_embedded.get(self._sequence_name + "_jagged")
        if jag is not None:
            limit = self.jagged_limit()
            if limit is not None:
                raise ValueError(f"{limit} (use the padded form)")
            max_len = int(sequence_embedded[self._sequence_name + "_max_len"])
            if self._max_seq_length > 0:
                max_len = min(max_len, self._max_seq_length)
            return jagged_pool(jag, sequence_embedded[self._sequence_name + "_offsets"], max_len, self._pooling_type)
        sequence = sequence_embedded[self._sequence_name]
        if self._max_seq_length > 0:
            sequence = sequence[:, : self._max_seq_length, :]
        feature = torch.sum(sequence, dim=1)
        if self._pooling_type == "mean":
            sequence_length = sequence_embedded[self._sequence_length_name]
            if self._max_seq_length > 0:
                sequence_length = torch.clamp_max(sequence_length, self._max_seq_length)
            # (a count is never more than the positions the tensor holds: the reference pads to the batch's longest sequence, so
            # there the clamp changes nothing; a group padded to its configured `sequence_length` truncates longer samples)
            feature = feature / torch.clamp(sequence_length, 1, max(sequence.size(1), 1)).unsqueeze(1)
        return feature


def encoder_jagged_limit(enc: nn.Module, max_len: int) -> Optional[str]:
    """None when `enc` evaluates a sequence group handed over as rows with padded length `max_len`, else why not"""
    if isinstance(enc, DINEncoder):
        lim = enc.jagged_limit()
        eff = min(max_len, enc._max_seq_length) if enc._max_seq_length > 0 else max_len
        if lim is None and eff > DIN_JAGGED_MAX_LEN:
            lim = f"max_len {eff} must be at most {DIN_JAGGED_MAX_LEN}"
        return lim
    return enc.jagged_limit(max_len)


def create_seq_encoder(spec, group_total_dim: Dict[str, int]) -> nn.Module:
    """The encoder module of one `config.SeqEncoderSpec` (the reference's create_seq_encoder, tzrec/modules/sequence.py:370-394);
    `group_total_dim`: "<sequence group>.query" / ".sequence" -> width."""
    sequence_dim, query_dim = group_total_dim[f"{spec.input}.sequence"], group_total_dim[f"{spec.input}.query"]
    if spec.kind == "din_encoder":
        return DINEncoder(sequence_dim, query_dim, spec.input, attn_mlp=dict(spec.attn_mlp), max_seq_length=spec.max_seq_length)
    if spec.kind == "simple_attention":
        return SimpleAttention(sequence_dim, query_dim, spec.input, max_seq_length=spec.max_seq_length)
    if spec.kind == "pooling_encoder":
        return PoolingEncoder(sequence_dim, spec.input, pooling_type=spec.pooling_type, max_seq_length=spec.max_seq_length)
    raise NotImplementedError(f"sequence encoder {spec.kind!r} is not built")
