"""WuKong (https://arxiv.org/abs/2403.02545) layers with the reference's parameters and state-dict keys
(tzrec/modules/interaction.py:236-378): `LinearCompressBlock`, `FactorizationMachineBlock`, `WuKongLayer`.

The GEMMs stay where they are (the FMB's MLP is `MLP`, so `_LinearReluFn` on the device; `feature_out_liner` is an `nn.Linear`).
Everything else of a layer is two per-sample operations on the kernels of csrc/wukong.hip, one autograd Function each:
`_WukongFmFn` (X^T W, X P and the LayerNorm over the F k values in front of the MLP) and `_WukongMixFn` (lcb, the residual
projection, the concat, the add and the LayerNorm over D behind it): 2 launches forward and 4 backward per layer, where the
literal form permutes [B, F, D] six times and keeps most of what it makes.  Autograd adds the two input gradients of a layer.
`FUSED_WUKONG = False`, or a shape, dtype or device the kernels refuse, runs the reference's literal forward.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch
from torch import nn

from . import _lib
from .dlrm import MLP
from .interaction import _traced

FUSED_WUKONG = True  # A/B switch: False = the reference's literal forward (permute, matmul, LayerNorm, concat, add, op by op)
WUKONG_MAX_F, WUKONG_MAX_D = 64, 128  # WK_MAXF (F, Fo and k), WK_MAXD of csrc/wukong.hip


class _WukongFmFn(torch.autograd.Function):
    """LN(vec(X (X^T W)); gamma, beta) [B, F k] of x [B, F, D] on tzr_wukong_fm_fwd / tzr_wukong_fm_bwd.
    Saved: the inputs and the [B, 2] statistics -- neither X^T W nor X P."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
        B, F, D = x.shape
        k = weight.shape[1]
        x2 = _lib.scalar_rows(x.reshape(B, F * D))
        weight, gamma, beta = weight.contiguous(), gamma.contiguous(), beta.contiguous()
        dev = x.device
        out = torch.empty(B, F * k, dtype=torch.float32, device=dev)
        stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
        rc = _lib.lib().tzr_wukong_fm_fwd(_lib.ptr(x2), _lib.scalar_row_stride(x2), _lib.ptr(weight), _lib.ptr(gamma), _lib.ptr(beta),
                                          eps, B, F, D, k, _lib.ptr(out), F * k, _lib.ptr(stats), _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_wukong_fm_fwd")
        ctx.save_for_backward(x2, weight, gamma, stats)
        ctx.dims = (B, F, D, k)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        x2, weight, gamma, stats = ctx.saved_tensors
        B, F, D, k = ctx.dims
        dev = x2.device
        gout = _lib.scalar_rows(gout)
        gx = torch.empty(B, F, D, dtype=torch.float32, device=dev)
        dp = torch.empty(3 * F * k, dtype=torch.float32, device=dev)
        lib = _lib.lib()
        ws = _lib.workspace(lib.tzr_wukong_fm_bwd_workspace(B, F, D, k), dev)
        rc = lib.tzr_wukong_fm_bwd(_lib.ptr(gout), _lib.scalar_row_stride(gout), _lib.ptr(x2), _lib.scalar_row_stride(x2),
                                   _lib.ptr(weight), _lib.ptr(gamma), _lib.ptr(stats), B, F, D, k, _lib.ptr(gx), F * D,
                                   _lib.ptr(dp), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_wukong_fm_bwd")
        n = F * k
        return gx, dp[:n].view(F, k), dp[n:2 * n], dp[2 * n:], None


class _WukongMixFn(torch.autograd.Function):
    """LN_D(concat(fm, X^T Wl) + X^T Wr) [B, Fo, D] (Wr None: + X) of x [B, F, D] and fm [B, Ff D] on tzr_wukong_mix_fwd /
    tzr_wukong_mix_bwd.  Saved: the inputs and the [B, Fo, 2] statistics -- no projection, no concat, no sum."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, fm: torch.Tensor, wl: torch.Tensor, wr: Optional[torch.Tensor], gamma: torch.Tensor,
                beta: torch.Tensor, eps: float):
        B, F, D = x.shape
        Fl = wl.shape[1]
        Ff = fm.shape[1] // D
        Fo = Ff + Fl
        x2, fm = _lib.scalar_rows(x.reshape(B, F * D)), _lib.scalar_rows(fm)
        wl, gamma, beta = wl.contiguous(), gamma.contiguous(), beta.contiguous()
        wr = None if wr is None else wr.contiguous()
        dev = x.device
        out = torch.empty(B, Fo, D, dtype=torch.float32, device=dev)
        stats = torch.empty(B, Fo, 2, dtype=torch.float32, device=dev)
        rc = _lib.lib().tzr_wukong_mix_fwd(_lib.ptr(x2), _lib.scalar_row_stride(x2), _lib.ptr(fm), _lib.scalar_row_stride(fm),
                                           _lib.ptr(wl), _lib.ptr(wr), _lib.ptr(gamma), _lib.ptr(beta), eps, B, F, D, Ff, Fl,
                                           _lib.ptr(out), Fo * D, _lib.ptr(stats), _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_wukong_mix_fwd")
        ctx.save_for_backward(x2, fm, wl, gamma, stats, *(() if wr is None else (wr,)))
        ctx.dims = (B, F, D, Ff, Fl)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        x2, fm, wl, gamma, stats, *rest = ctx.saved_tensors
        wr = rest[0] if rest else None
        B, F, D, Ff, Fl = ctx.dims
        Fo = Ff + Fl
        dev = x2.device
        gout = _lib.scalar_rows(gout.reshape(B, Fo * D))
        gx = torch.empty(B, F, D, dtype=torch.float32, device=dev)
        gfm = torch.empty(B, Ff * D, dtype=torch.float32, device=dev)
        dp = torch.empty(F * Fo + F * Fl + 2 * D, dtype=torch.float32, device=dev)
        lib = _lib.lib()
        ws = _lib.workspace(lib.tzr_wukong_mix_bwd_workspace(B, F, D, Ff, Fl), dev)
        rc = lib.tzr_wukong_mix_bwd(_lib.ptr(gout), _lib.scalar_row_stride(gout), _lib.ptr(x2), _lib.scalar_row_stride(x2), _lib.ptr(fm),
                                    _lib.scalar_row_stride(fm), _lib.ptr(wl), _lib.ptr(wr), _lib.ptr(gamma), _lib.ptr(stats),
                                    B, F, D, Ff, Fl, _lib.ptr(gx), F * D, _lib.ptr(gfm), Ff * D, _lib.ptr(dp), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_wukong_mix_bwd")
        a, b = F * Fo, F * Fo + F * Fl
        return gx, gfm, dp[a:b].view(F, Fl), (None if wr is None else dp[:a].view(F, Fo)), dp[b:b + D], dp[b + D:], None


def wukong_ok(x: torch.Tensor, *params: torch.Tensor) -> bool:
    """the kernels take `x` [B, F, D] with these parameters"""
    return bool(x.dim() == 3 and x.dtype == torch.float32 and x.shape[0] > 0 and not _traced(x)
                and 1 <= x.shape[1] <= WUKONG_MAX_F and 1 <= x.shape[2] <= WUKONG_MAX_D
                and all(p.dtype == torch.float32 for p in params) and (x.is_cuda or _lib.emulated()))


class LinearCompressBlock(nn.Module):
    """[B, F_in, D] -> [B, F_out, D]: a weight [F_in, F_out] over the feature axis (interaction.py:236-264)."""

    def __init__(self, feature_num_in: int, feature_num_out: int) -> None:
        super().__init__()
        self._feature_num_out = feature_num_out
        self._feature_num_in = feature_num_in
        self.weight = nn.Parameter(torch.empty((feature_num_in, feature_num_out)))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.weight)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        return (inputs.permute(0, 2, 1) @ self.weight).permute(0, 2, 1)


class FactorizationMachineBlock(nn.Module):
    """The optimised FM of WuKong (interaction.py:267-321): X (X^T W) flattened to [B, F_in k], LayerNorm, an MLP and a Linear
    to `feature_num_out` rows of width `input_dim`."""

    def __init__(self, input_dim: int, feature_num_in: int, feature_num_out: int, compressed_feature_num: int,
                 feature_num_mlp: Optional[Dict[str, Any]] = None) -> None:
        super().__init__()
        self.feature_num_in = feature_num_in
        self.feature_num_out = feature_num_out
        self.input_dim = input_dim
        self.compressed_feature_num = compressed_feature_num
        self.weight = nn.Parameter(torch.empty((feature_num_in, compressed_feature_num)))
        self.norm = nn.LayerNorm(feature_num_in * compressed_feature_num)
        self.mlp = MLP(in_features=feature_num_in * compressed_feature_num, **(feature_num_mlp or {}))
        self.feature_out_liner = nn.Linear(self.mlp.output_dim(), self.feature_num_out * self.input_dim)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.weight)

    def _fused_ok(self, x: torch.Tensor) -> bool:
        return FUSED_WUKONG and self.compressed_feature_num <= WUKONG_MAX_F and wukong_ok(x, self.weight, self.norm.weight, self.norm.bias)

    def tail(self, normed: torch.Tensor) -> torch.Tensor:
        """[B, F_in k] behind the LayerNorm -> [B, F_out D]"""
        return self.feature_out_liner(self.mlp(normed))

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        if self._fused_ok(inputs):
            outputs = _WukongFmFn.apply(inputs, self.weight, self.norm.weight, self.norm.bias, self.norm.eps)
        else:  # the reference's literal form
            outputs = torch.matmul(inputs, torch.matmul(inputs.permute(0, 2, 1), self.weight))
            outputs = self.norm(outputs.view(-1, self.feature_num_in * self.compressed_feature_num))
        return self.tail(outputs).view(-1, self.feature_num_out, self.input_dim)


class WuKongLayer(nn.Module):
    """LN(concat(fmb(x), lcb(x)) + residual_projection(x)) (interaction.py:324-378); the residual is the identity when the
    layer keeps the number of features."""

    def __init__(self, input_dim: int, feature_num: int, lcb_feature_num: int, fmb_feature_num: int, compressed_feature_num: int,
                 feature_num_mlp: Optional[Dict[str, Any]] = None) -> None:
        super().__init__()
        self.lcb_feature_num = lcb_feature_num
        self.fmb_feature_num = fmb_feature_num
        self.lcb = LinearCompressBlock(feature_num, lcb_feature_num)
        self.fmb = FactorizationMachineBlock(input_dim, feature_num, fmb_feature_num, compressed_feature_num, feature_num_mlp)
        self.norm = nn.LayerNorm(input_dim)
        if feature_num != lcb_feature_num + fmb_feature_num:
            self.residual_projection = LinearCompressBlock(feature_num, lcb_feature_num + fmb_feature_num)
        else:
            self.residual_projection = nn.Identity()

    def output_feature_num(self) -> int:
        return self.lcb_feature_num + self.fmb_feature_num

    def _fused_ok(self, x: torch.Tensor) -> bool:
        wr = getattr(self.residual_projection, "weight", None)
        return bool(self.fmb._fused_ok(x) and self.lcb_feature_num >= 1 and self.fmb_feature_num >= 1
                    and self.output_feature_num() <= WUKONG_MAX_F
                    and wukong_ok(x, self.lcb.weight, self.norm.weight, self.norm.bias, *(() if wr is None else (wr,)))
                    and all(p.dtype == torch.float32 for p in self.fmb.parameters()))

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        if self._fused_ok(inputs):
            fmb, B = self.fmb, inputs.shape[0]
            fm = fmb.tail(_WukongFmFn.apply(inputs, fmb.weight, fmb.norm.weight, fmb.norm.bias, fmb.norm.eps))
            wr = getattr(self.residual_projection, "weight", None)
            return _WukongMixFn.apply(inputs, fm.view(B, -1), self.lcb.weight, wr, self.norm.weight, self.norm.bias, self.norm.eps)
        outputs = torch.concat((self.fmb(inputs), self.lcb(inputs)), dim=1)  # the reference's literal form
        return self.norm(outputs + self.residual_projection(inputs))
