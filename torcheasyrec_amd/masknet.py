"""MaskNet (https://arxiv.org/pdf/2102.07619) with the reference's parameters and state-dict keys
(tzrec/modules/masknet.py:20-161): `MaskBlock` and `MaskNetModule`.

The GEMMs stay where they are (`nn.Linear`; `_LinearReluFn` for the mask generator's `Linear -> ReLU` on the device).
Everything between them -- `LayerNorm(x) * mask_i` in front of every block, `LayerNorm -> ReLU` behind every block's
hidden layer, the parallel blocks' concat -- runs on the row kernels of csrc/ln_mask.hip through one autograd Function:
2 row launches each way for any number of parallel blocks, n + 1 for n serial blocks.  `FUSED_MASKNET = False`, or a
shape, dtype or device the kernels refuse, runs the reference's literal loop.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence

import torch
from torch import nn

from . import _lib
from .dlrm import MLP, _LinearReluFn
from .interaction import _traced

FUSED_MASKNET = True  # A/B switch: False = the reference's literal loop (nn.LayerNorm, a multiply, nn.ReLU, a concat, op by op)
LN_MASK_MAX_DIM, LN_MASK_MAX_OUT = 1024, 8  # LM_MAXDIM, LM_MAXOUT of csrc/ln_mask.hip


def _strides(ts: Sequence[torch.Tensor]):
    return (C.c_int64 * len(ts))(*[_lib.scalar_row_stride(t) for t in ts])


class _LnMaskFn(torch.autograd.Function):
    """out_j = act(LN(x_j; gamma_j, beta_j)) [* m_j] for j < n_out on tzr_ln_mask_fwd / tzr_ln_mask_bwd.  `shared`: one x,
    gamma, beta for every j.  `concat`: the outputs are the column blocks of ONE [B, n_out D] tensor, which is what is
    returned (and whose gradient's column blocks the backward reads as they lie); otherwise n_out tensors are returned.
    Tensor arguments: n_x rows x, n_x gammas, n_x betas, then n_out masks or none (n_x = 1 when shared, else n_out).
    Saved: the inputs and the [B, n_x, 2] statistics -- neither LN(x) nor any output."""

    @staticmethod
    def forward(ctx, n_out: int, shared: bool, relu: bool, concat: bool, eps: float, *ts: torch.Tensor):
        n_x = 1 if shared else n_out
        xs = [_lib.scalar_rows(t) for t in ts[:n_x]]
        gammas = [t.contiguous() for t in ts[n_x:2 * n_x]]
        betas = [t.contiguous() for t in ts[2 * n_x:3 * n_x]]
        ms = [_lib.scalar_rows(t) for t in ts[3 * n_x:]]
        assert len(ms) in (0, n_out)
        B, D = xs[0].shape
        dev = xs[0].device
        buf = torch.empty(B, n_out * D, dtype=torch.float32, device=dev)
        outs = [buf[:, j * D:(j + 1) * D] for j in range(n_out)]
        stats = torch.empty(B, n_x, 2, dtype=torch.float32, device=dev)
        rc = _lib.lib().tzr_ln_mask_fwd(_lib.ptr_array(xs), _strides(xs), _lib.ptr_array(gammas), _lib.ptr_array(betas), _lib.ptr_array(ms) if ms else None,
                                        _strides(ms) if ms else None, _lib.ptr_array(outs), _strides(outs), n_out, int(shared), int(relu),
                                        eps, B, D, _lib.ptr(stats), _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_ln_mask_fwd")
        ctx.save_for_backward(stats, *xs, *gammas, *betas, *ms)
        ctx.cfg = (n_out, n_x, bool(shared), bool(relu), bool(concat), len(ms) > 0)
        if concat or n_out == 1:
            return buf
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts: torch.Tensor):
        n_out, n_x, shared, relu, concat, masked = ctx.cfg
        stats, *ts = ctx.saved_tensors
        xs, gammas, betas, ms = ts[:n_x], ts[n_x:2 * n_x], ts[2 * n_x:3 * n_x], ts[3 * n_x:]
        B, D = xs[0].shape
        dev = xs[0].device
        if concat or n_out == 1:
            g = _lib.scalar_rows(gouts[0])
            gouts = [g[:, j * D:(j + 1) * D] for j in range(n_out)]
        else:
            gouts = [_lib.scalar_rows(g) for g in gouts]
        gx = [torch.empty(B, D, dtype=torch.float32, device=dev) for _ in range(n_x)]
        gm = [torch.empty(B, D, dtype=torch.float32, device=dev) for _ in range(n_out)] if masked else []
        dgb = torch.empty(2, n_x, D, dtype=torch.float32, device=dev)
        lib = _lib.lib()
        ws = _lib.workspace(lib.tzr_ln_mask_bwd_workspace(B, D, n_out, int(shared)), dev)
        rc = lib.tzr_ln_mask_bwd(_lib.ptr_array(gouts), _strides(gouts), _lib.ptr_array(xs), _strides(xs), _lib.ptr_array(gammas), _lib.ptr_array(betas),
                                 _lib.ptr_array(ms) if masked else None, _strides(ms) if masked else None, _lib.ptr(stats), n_out,
                                 int(shared), int(relu), B, D, _lib.ptr_array(gx), _strides(gx), _lib.ptr_array(gm) if masked else None,
                                 _strides(gm) if masked else None, _lib.ptr(dgb[0]), _lib.ptr(dgb[1]), _lib.ptr(ws), ws.numel(),
                                 _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_ln_mask_bwd")
        return (None, None, None, None, None, *gx, *[dgb[0, j] for j in range(n_x)], *[dgb[1, j] for j in range(n_x)], *gm)


def ln_mask_ok(x: torch.Tensor, n_out: int, *params: torch.Tensor) -> bool:
    """the row kernels take `x` [B, D] with these LayerNorm parameters for n_out outputs"""
    return bool(x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] > 0 and not _traced(x)
                and 1 <= x.shape[1] <= LN_MASK_MAX_DIM and 1 <= n_out <= LN_MASK_MAX_OUT
                and all(p is not None and p.dtype == torch.float32 for p in params) and (x.is_cuda or _lib.emulated()))


def _linear_relu(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda and x.dtype == torch.float32 and lin.bias is not None and not _traced(x):
        return _LinearReluFn.apply(x, lin.weight, lin.bias)  # the ReLU in the GEMM's epilogue
    return torch.relu(lin(x))


class MaskBlock(nn.Module):
    """One mask block, the reference's constructor as it behaves (masknet.py:33-71): `aggregation_dim` is
    `int(input_dim * reduction_ratio)` whenever `reduction_ratio` is non-zero -- of the block's FEATURE input, which in serial
    mode is the previous block's hidden width -- and the configured `aggregation_dim` counts only with `reduction_ratio` 0."""

    def __init__(self, input_dim: int, mask_input_dim: int, hidden_dim: int, reduction_ratio: float = 1.0,
                 aggregation_dim: int = 0) -> None:
        super().__init__()
        if not aggregation_dim and not reduction_ratio:
            raise ValueError("Either aggregation_dim or reduction_ratio must be provided.")
        if aggregation_dim:
            self.aggregation_dim = aggregation_dim
        if reduction_ratio:
            self.aggregation_dim = int(input_dim * reduction_ratio)
        assert self.aggregation_dim > 0, "aggregation_dim must be > 0, check your aggregation_dim or reduction_ratio settings."
        self.mask_generator = nn.Sequential(nn.Linear(mask_input_dim, self.aggregation_dim), nn.ReLU(),
                                            nn.Linear(self.aggregation_dim, input_dim))
        assert hidden_dim > 0, "hidden_dim must be > 0."
        self._hidden_dim = hidden_dim
        self.ffn = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.LayerNorm(hidden_dim), nn.ReLU())

    def output_dim(self) -> int:
        return self._hidden_dim

    def mask(self, mask_input: torch.Tensor) -> torch.Tensor:
        return self.mask_generator[2](_linear_relu(self.mask_generator[0], mask_input))

    def forward(self, feature_input: torch.Tensor, mask_input: torch.Tensor) -> torch.Tensor:
        return self.ffn(feature_input * self.mask_generator(mask_input))  # the reference's literal form


class MaskNetModule(nn.Module):
    """`ln_emb`, `n_mask_blocks` mask blocks side by side over LN(x) (parallel: their outputs concatenated) or one after the
    other (serial: block i masks the hidden state of block i - 1), an optional `top_mlp` (masknet.py:88-161)."""

    def __init__(self, feature_dim: int, n_mask_blocks: int, mask_block: Dict[str, Any], top_mlp: Optional[Dict[str, Any]] = None,
                 use_parallel: bool = True) -> None:
        super().__init__()
        self.ln_emb = nn.LayerNorm(feature_dim)
        self.use_parallel = use_parallel
        if use_parallel:
            self.mask_blocks = nn.ModuleList([MaskBlock(feature_dim, feature_dim, **mask_block) for _ in range(n_mask_blocks)])
            self._output_dim = self.mask_blocks[0].output_dim() * n_mask_blocks
        else:
            self.mask_blocks = nn.ModuleList()
            self._output_dim = feature_dim
            for i in range(n_mask_blocks):
                self.mask_blocks.append(MaskBlock(self._output_dim, feature_dim, **mask_block))
                self._output_dim = self.mask_blocks[i].output_dim()
        self.top_mlp = None
        if top_mlp:
            self.top_mlp = MLP(in_features=self._output_dim, **top_mlp)
            self._output_dim = self.top_mlp.output_dim()

    def output_dim(self) -> int:
        return self._output_dim

    def _layer_norms(self) -> List[nn.LayerNorm]:
        return [self.ln_emb] + [b.ffn[1] for b in self.mask_blocks]

    def _fused_ok(self, x: torch.Tensor) -> bool:
        n = len(self.mask_blocks)
        lns = self._layer_norms()
        if not (FUSED_MASKNET and n >= 1 and ln_mask_ok(x, n if self.use_parallel else 1, *[p for ln in lns for p in (ln.weight, ln.bias)])):
            return False
        if max(ln.normalized_shape[0] for ln in lns) > LN_MASK_MAX_DIM:
            return False
        return all(p.dtype == torch.float32 for b in self.mask_blocks for p in b.parameters())

    def _fused(self, x: torch.Tensor) -> torch.Tensor:
        blocks, ln0, n = self.mask_blocks, self.ln_emb, len(self.mask_blocks)
        if self.use_parallel:
            masks = [b.mask(x) for b in blocks]
            w = _LnMaskFn.apply(n, True, False, False, ln0.eps, x, ln0.weight, ln0.bias, *masks)
            w = (w,) if n == 1 else w
            z = [b.ffn[0](wi) for b, wi in zip(blocks, w)]
            lns = [b.ffn[1] for b in blocks]
            eps = lns[0].eps  # (one constructor: every block's LayerNorm has the default eps)
            return _LnMaskFn.apply(n, False, True, True, eps, *z, *[l.weight for l in lns], *[l.bias for l in lns])
        w = _LnMaskFn.apply(1, True, False, False, ln0.eps, x, ln0.weight, ln0.bias, blocks[0].mask(x))
        for i in range(n):
            z, ln = blocks[i].ffn[0](w), blocks[i].ffn[1]
            nxt = (blocks[i + 1].mask(x),) if i + 1 < n else ()  # (the hidden state between two blocks is never written)
            w = _LnMaskFn.apply(1, False, True, False, ln.eps, z, ln.weight, ln.bias, *nxt)
        return w

    def forward(self, feature_emb: torch.Tensor) -> torch.Tensor:
        if self._fused_ok(feature_emb):
            hidden = self._fused(feature_emb)
        else:  # the reference's literal form
            ln_emb = self.ln_emb(feature_emb)
            if self.use_parallel:
                hidden = torch.concat([b(ln_emb, feature_emb) for b in self.mask_blocks], dim=-1)
            else:
                hidden = self.mask_blocks[0](ln_emb, feature_emb)
                for i in range(1, len(self.mask_blocks)):
                    hidden = self.mask_blocks[i](hidden, feature_emb)
        if self.top_mlp is not None:
            hidden = self.top_mlp(hidden)
        return hidden
