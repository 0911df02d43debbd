"""One fused sparse backward, described once: the only place that knows the argument order of `tzr_pooled_bwd_*`.

The C entry points (include/tzrec_hip.h) take 13-20 positional arguments each, most of them the same description of one
problem -- which tables, which lookups, which ids, how many positions -- and ctypes checks none of their order.
`SparseBackward` holds that description under names; its methods are the calls.  Every caller (the pooled and the sequence
collections, both halves of the sharded one, the torch.library ops) builds one per batch and says what it wants done.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib


def grad_dsts(tensors: Sequence[torch.Tensor]):
    """TzrDst[len(tensors)]: pointer and row stride of every [B, width] destination (pooled outputs, or their gradients).  The
    array holds addresses only: the caller keeps the tensors alive over the launch."""
    arr = (_lib.TzrDst * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i].ptr, arr[i].stride = _lib.ptr(t), t.stride(0)
    return arr


def cells_geometry(h_tables: np.ndarray, h_feats: np.ndarray, B: int, max_dim: int):
    """(image, info8) of tzr_bwd_cells_geometry for the HOST copies of a backward's descriptors at batch size B: the uint8 image
    the cells launchers read their header from, and what the library says about it.  None: not a case for the cells plan.
    The arrays' lengths are the call's n_tables and n_feats: pass whole descriptor arrays, one record per table / lookup."""
    L, info = _lib.lib(), (C.c_int64 * 8)()
    args = (h_tables.ctypes.data, len(h_tables), h_feats.ctypes.data, len(h_feats), B, max_dim)
    rc = L.tzr_bwd_cells_geometry(*args, None, 0, info)
    if rc == _lib.TZR_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "tzr_bwd_cells_geometry")
    img = np.zeros(int(info[0]), dtype=np.uint8)
    _lib.check(L.tzr_bwd_cells_geometry(*args, img.ctypes.data, img.nbytes, info), "tzr_bwd_cells_geometry")
    return img, info


def direct_supported(n_positions: int, n_feats: int, n_tables: int, uniform: bool, grad_mode: int = 0) -> bool:
    """whether the library takes a backward of this shape and size in ONE launch (tzr_tune "bwd_direct"): a question about
    sizes alone, asked before descriptors or ids exist"""
    return bool(_lib.lib().tzr_pooled_bwd_direct_supported(n_positions, n_feats, n_tables, 1 if uniform else 0, grad_mode))


@dataclass(slots=True)
class SparseBackward:
    """The fused backward of one batch: K6 (index plan) + K7 (per-row gradient sums and the optimizer), in any of its forms.
    `plan` + `apply`: the four-launch plan, any ids; `cells_plan` + `cells_apply`: the one-launch plan of batches with one id per
    bag (`geo`: its geometry, host header `h_ptr` + device image `d_img`); `direct`: one launch, no plan, where
    `direct_supported()`.  `grads` is a `grad_dsts` array, `opt` a TzrSparseOptim."""

    device: torch.device
    d_tables: torch.Tensor  # TzrTable[n_tables] / TzrFeature[n_feats], the backward's (frozen lookups masked)
    d_feats: torch.Tensor
    n_tables: int
    n_feats: int
    n_keys: int
    max_rows: int
    max_dim: int
    values: torch.Tensor
    offsets: Optional[torch.Tensor]  # None: every bag holds exactly one id (the calls' `uniform_bag_len`)
    weights: Optional[torch.Tensor]
    n_values: int
    n_positions: int  # capacity of the table-major position space
    B: int
    grad_mode: int = 0  # 0: gradients of the pooled outputs; 1: one gradient row per id

    # -- sizes and questions: no launch ------------------------------------------------------------------------------
    def plan_bytes(self) -> int:
        return _lib.lib().tzr_pooled_bwd_workspace(self.n_values, self.n_positions, self.n_feats, self.n_tables, self.B, self.max_dim)

    def direct_supported(self) -> bool:
        return direct_supported(self.n_positions, self.n_feats, self.n_tables, self.offsets is None, self.grad_mode)

    def direct_bytes(self) -> int:
        return _lib.lib().tzr_pooled_bwd_direct_workspace(self.n_positions, self.n_tables, self.max_dim)

    # -- K6 ----------------------------------------------------------------------------------------------------------
    def plan(self, ws: torch.Tensor) -> None:
        p = _lib.ptr
        _lib.check(_lib.lib().tzr_pooled_bwd_plan(
            p(self.d_tables), self.n_tables, p(self.d_feats), self.n_feats, self.n_keys, self.max_rows, self.max_dim,
            p(self.values), p(self.offsets), self.n_values, self.n_positions, self.B, 1 if self.offsets is None else 0,
            p(ws), ws.numel(), _lib.stream_ptr(self.device)), "tzr_pooled_bwd_plan")

    def cells_plan(self, geo, ws: torch.Tensor) -> None:
        p = _lib.ptr
        _lib.check(_lib.lib().tzr_pooled_bwd_cells_plan(
            p(self.d_tables), self.n_tables, p(self.d_feats), self.n_feats, self.max_dim, p(self.values), self.n_values, self.B,
            geo.h_ptr, p(geo.d_img), p(ws), ws.numel(), _lib.stream_ptr(self.device)), "tzr_pooled_bwd_cells_plan")

    # -- K7 ----------------------------------------------------------------------------------------------------------
    def apply(self, ws: torch.Tensor, grads, opt) -> None:
        p = _lib.ptr
        _lib.check(_lib.lib().tzr_pooled_bwd_apply(
            p(self.d_tables), p(self.d_feats), self.n_feats, self.n_tables, self.max_dim, p(self.offsets), p(self.weights),
            self.n_values, self.n_positions, self.B, 1 if self.offsets is None else 0, self.grad_mode, grads, len(grads), opt,
            p(ws), ws.numel(), _lib.stream_ptr(self.device)), "tzr_pooled_bwd_apply")

    def cells_apply(self, geo, ws: torch.Tensor, grads, opt) -> None:
        p = _lib.ptr
        _lib.check(_lib.lib().tzr_pooled_bwd_cells_apply(
            p(self.d_tables), p(self.d_feats), self.n_feats, self.n_tables, self.max_dim, p(self.weights), self.n_values, self.B,
            self.grad_mode, grads, len(grads), opt, geo.h_ptr, p(geo.d_img), p(ws), ws.numel(), _lib.stream_ptr(self.device)),
            "tzr_pooled_bwd_cells_apply")

    def direct(self, ws: torch.Tensor, grads, opt, hot_rows: bool = False) -> None:
        """`ws`: `direct_bytes()` of zeroed, KEPT memory (the kernel's arrival counters reset themselves); `hot_rows`: a row
        with more lookups than a workgroup's LDS holds is expected (TZR_GRAD_HOT_ROWS)"""
        p = _lib.ptr
        _lib.check(_lib.lib().tzr_pooled_bwd_direct(
            p(self.d_tables), self.n_tables, p(self.d_feats), self.n_feats, self.max_rows, self.max_dim, p(self.values),
            p(self.offsets), p(self.weights), self.n_values, self.n_positions, self.B, 1 if self.offsets is None else 0,
            self.grad_mode | (_lib.GRAD_HOT_ROWS if hot_rows else 0), grads, len(grads), opt, p(ws), ws.numel(),
            _lib.stream_ptr(self.device)), "tzr_pooled_bwd_direct")
