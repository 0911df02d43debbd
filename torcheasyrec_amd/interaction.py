"""Feature-interaction modules on the gfx950 kernels.

``InteractionArch`` and ``FactorizationMachine`` keep the reference's constructor and ``forward``
(/root/reference/tzrec/modules/interaction.py:57-91, /root/reference/tzrec/modules/fm.py:17-42).
``dot_interaction`` is the fused form DLRM uses here: it reads the dense-MLP output and the pooled
sparse block separately (no ``cat`` to build [B, 27, 16]) and writes
``[interactions | dense | sparse]`` in one pass (/root/reference/tzrec/models/dlrm.py:123-130).
``Cross`` is the cross network of Deep & Cross v1 with the reference's parameters (interaction.py:94-132), every layer
of it in one launch per direction (csrc/cross_net.hip).
``CrossV2`` is the low-rank cross network of Deep & Cross v2 with the reference's parameters (interaction.py:135-180), every
layer of it in one launch forward and two backward (csrc/cross_v2.hip).
``CIN`` is the compressed interaction network of xDeepFM with the reference's parameters (interaction.py:183-233); the
[B, H F, D] product tensor the reference builds per layer never exists (csrc/cin.hip).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _lib
from . import ops as _ops  # noqa: F401  (registers torch.ops.tzrec_hip.*)


def _traced(t: torch.Tensor) -> bool:
    """True when `t` is being traced (FX / make_fx / dynamo / torch.export: fake or proxy tensors).  Traced
    programs go through `torch.ops.tzrec_hip.*` so the graph shows the ops; eager calls keep
    the direct autograd.Function path below, which costs no dispatcher round trip per call."""
    return torch.compiler.is_compiling() or type(t) not in (torch.Tensor, nn.Parameter)


class _DotInteractionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dense: Optional[torch.Tensor], sparse: torch.Tensor, D: int, cat_dense: bool, cat_sparse: bool):
        B = sparse.shape[0]
        F = sparse.shape[1] // D
        sparse = sparse.contiguous()
        if dense is not None:
            dense = dense.contiguous()
        n = F + (1 if dense is not None else 0)
        width = n * (n - 1) // 2 + (D if (cat_dense and dense is not None) else 0) + (F * D if cat_sparse else 0)
        out = torch.empty(B, width, dtype=torch.float32, device=sparse.device)
        rc = _lib.lib().tzr_dot_interaction_fwd(
            _lib.ptr(dense), dense.stride(0) if dense is not None else 0, _lib.ptr(sparse),
            sparse.stride(0), F, D, B, _lib.ptr(out), out.stride(0), int(cat_dense), int(cat_sparse),
            _lib.stream_ptr(sparse.device),
        )
        _lib.check(rc, "tzr_dot_interaction_fwd")
        ctx.save_for_backward(dense, sparse)
        ctx.cfg = (F, D, cat_dense, cat_sparse)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        dense, sparse = ctx.saved_tensors
        F, D, cat_dense, cat_sparse = ctx.cfg
        B = sparse.shape[0]
        gout = gout.contiguous()
        gs = torch.empty_like(sparse)
        gd = torch.empty_like(dense) if dense is not None else None
        rc = _lib.lib().tzr_dot_interaction_bwd(
            _lib.ptr(dense), dense.stride(0) if dense is not None else 0, _lib.ptr(sparse),
            sparse.stride(0), F, D, B, _lib.ptr(gout), gout.stride(0), int(cat_dense),
            int(cat_sparse), _lib.ptr(gd), gd.stride(0) if gd is not None else 0, _lib.ptr(gs),
            gs.stride(0), _lib.stream_ptr(sparse.device),
        )
        _lib.check(rc, "tzr_dot_interaction_bwd")
        return gd, gs, None, None, None


def dot_interaction(
    dense: Optional[torch.Tensor], sparse: torch.Tensor, dim: int, cat_dense: bool = True, cat_sparse: bool = True
) -> torch.Tensor:
    """[B, n(n-1)/2 (+dim) (+F*dim)]: strict-upper-triangle of X X^T for X = [dense; sparse rows]."""
    if _traced(sparse):
        return torch.ops.tzrec_hip.dot_interaction_fwd(dense, sparse, dim, cat_dense, cat_sparse)
    return _DotInteractionFn.apply(dense, sparse, dim, cat_dense, cat_sparse)


class InteractionArch(nn.Module):
    """Feature interaction module (same signature as the reference: ``feature_num``; input
    ``B x N x D``; output ``B x N(N-1)/2``)."""

    def __init__(self, feature_num: int) -> None:
        super().__init__()
        self.feature_num = feature_num

    def output_dim(self) -> int:
        return self.feature_num * (self.feature_num - 1) // 2

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        B, N, D = features.shape
        return dot_interaction(None, features.reshape(B, N * D), D, False, False)


class _FMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor):
        B, F, D = x.shape
        x = x.contiguous()
        out = torch.empty(B, D, dtype=torch.float32, device=x.device)
        rc = _lib.lib().tzr_fm_fwd(_lib.ptr(x), x.stride(0), F, D, B, _lib.ptr(out), out.stride(0), _lib.stream_ptr(x.device))
        _lib.check(rc, "tzr_fm_fwd")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        (x,) = ctx.saved_tensors
        B, F, D = x.shape
        gout = gout.contiguous()
        gx = torch.empty_like(x)
        rc = _lib.lib().tzr_fm_bwd(
            _lib.ptr(x), x.stride(0), F, D, B, _lib.ptr(gout), gout.stride(0), _lib.ptr(gx), gx.stride(0), _lib.stream_ptr(x.device)
        )
        _lib.check(rc, "tzr_fm_bwd")
        return gx


class FactorizationMachine(nn.Module):
    """FM second-order term: [B, N, D] -> [B, D] (same signature as the reference)."""

    def forward(self, feature: torch.Tensor) -> torch.Tensor:
        if _traced(feature):
            return torch.ops.tzrec_hip.fm_fwd(feature)
        return _FMFn.apply(feature)


FUSED_CROSS = True  # A/B switch: False = the reference's literal loop (a product, a multiply and two adds per layer)
CROSS_MAX_DIM, CROSS_MAX_LAYERS = 1024, 8  # CN_MAXDIM, CN_MAXL of csrc/cross_net.hip


class _CrossFn(torch.autograd.Function):
    """y = x_L of x_{l+1} = (x_l . w_l) x_0 + b_l + x_l: tzr_cross_fwd keeps the scalars x_l . w_l ([B, L]), tzr_cross_bwd
    returns the input gradient and the finished gradients of every w_l and b_l (rows of one [2, L, D] buffer)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, L: int, *params: torch.Tensor):
        x = _lib.scalar_rows(x)
        B, D = x.shape
        params = tuple(p if p.is_contiguous() else p.contiguous() for p in params)
        y = torch.empty(B, D, dtype=torch.float32, device=x.device)
        s = torch.empty(B, L, dtype=torch.float32, device=x.device)
        rc = _lib.lib().tzr_cross_fwd(_lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr_array(params[:L]), _lib.ptr_array(params[L:]), L, B, D,
                                      _lib.ptr(y), D, _lib.ptr(s), _lib.stream_ptr(x.device))
        _lib.check(rc, "tzr_cross_fwd")
        ctx.save_for_backward(x, s, *params)
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        x, s, *params = ctx.saved_tensors
        B, D = x.shape
        L = len(params) // 2
        gy = _lib.scalar_rows(gy)
        dx = torch.empty(B, D, dtype=torch.float32, device=x.device)
        dwb = torch.empty(2, L, D, dtype=torch.float32, device=x.device)
        lib = _lib.lib()
        ws = _lib.workspace(lib.tzr_cross_bwd_workspace(B, D, L), x.device)
        rc = lib.tzr_cross_bwd(_lib.ptr(gy), _lib.scalar_row_stride(gy), _lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr(s),
                               _lib.ptr_array(params[:L]), _lib.ptr_array(params[L:]), L, B, D, _lib.ptr(dx), D,
                               _lib.ptr(dwb[0]), _lib.ptr(dwb[1]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
        _lib.check(rc, "tzr_cross_bwd")
        return (dx, None, *[dwb[0, l].view(1, D) for l in range(L)], *[dwb[1, l] for l in range(L)])


class Cross(nn.Module):
    """Cross layers of the Deep & Cross network (https://arxiv.org/pdf/1708.05123), the reference module's constructor,
    parameters and forward (tzrec/modules/interaction.py:94-132): `w.<i>.weight` [1, input_dim], `b.<i>` [input_dim]."""

    def __init__(self, input_dim: int, cross_num: int = 3) -> None:
        super().__init__()
        self.cross_num = cross_num
        self._input_dim = input_dim
        self.w = nn.ModuleList()
        self.b = nn.ParameterList()
        for _ in range(cross_num):
            self.w.append(nn.Linear(input_dim, 1, bias=False))
            self.b.append(nn.Parameter(torch.empty(input_dim)))
        self.reset_parameters()

    def output_dim(self) -> int:
        return self._input_dim

    def reset_parameters(self) -> None:
        for i in range(self.cross_num):
            nn.init.xavier_uniform_(self.w[i].weight)
            nn.init.zeros_(self.b[i])

    def _fused_ok(self, x: torch.Tensor) -> bool:
        return bool(FUSED_CROSS and x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] > 0 and not _traced(x)
                    and 1 <= self.cross_num <= CROSS_MAX_LAYERS and 1 <= x.shape[1] <= CROSS_MAX_DIM
                    and self.w[0].weight.dtype == torch.float32 and (x.is_cuda or _lib.emulated()))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fused_ok(x):
            return _CrossFn.apply(x, self.cross_num, *[m.weight for m in self.w], *self.b)
        x1 = x
        for i in range(self.cross_num):  # the reference's literal form
            x1 = self.w[i](x1) * x + self.b[i] + x1
        return x1


FUSED_CROSS_V2 = True  # A/B switch: False = the reference's literal loop (two GEMMs, a bias add, a multiply and an add per layer)
CROSS_V2_MAX_DIM, CROSS_V2_MAX_RANK, CROSS_V2_MAX_LAYERS = 1024, 64, 8  # CV_MAXDIM, CV_MAXR, CV_MAXL of csrc/cross_v2.hip


class _CrossV2Fn(torch.autograd.Function):
    """y = x_L of x_{l+1} = x_0 * (x_l U_l^T V_l^T + c_l) + x_l: tzr_cross_v2_fwd keeps x_1 .. x_{L-1} ([L-1, B, D]) and every
    t_l = x_l U_l^T ([L, B, r]) -- nothing when `save` is false (no gradient will be asked for); tzr_cross_v2_bwd returns the input gradient and the
    finished gradients of every U_l, V_l and c_l (slices of three buffers)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, L: int, save: bool, *params: torch.Tensor):
        x = _lib.scalar_rows(x)
        B, D = x.shape
        params = tuple(p if p.is_contiguous() else p.contiguous() for p in params)
        R = params[0].shape[0]
        y = torch.empty(B, D, dtype=torch.float32, device=x.device)
        xs = torch.empty(L - 1, B, D, dtype=torch.float32, device=x.device) if save else None
        t = torch.empty(L, B, R, dtype=torch.float32, device=x.device) if save else None
        rc = _lib.lib().tzr_cross_v2_fwd(_lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr_array(params[:L]), _lib.ptr_array(params[L:2 * L]),
                                         _lib.ptr_array(params[2 * L:]), L, B, D, R, _lib.ptr(y), D, _lib.ptr(xs), _lib.ptr(t),
                                         _lib.stream_ptr(x.device))
        _lib.check(rc, "tzr_cross_v2_fwd")
        if save:
            ctx.save_for_backward(x, xs, t, *params)
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        x, xs, t, *params = ctx.saved_tensors
        B, D = x.shape
        L = len(params) // 3
        R = params[0].shape[0]
        gy = _lib.scalar_rows(gy)
        dev = x.device
        dx = torch.empty(B, D, dtype=torch.float32, device=dev)
        du = torch.empty(L, R, D, dtype=torch.float32, device=dev)
        dv = torch.empty(L, D, R, dtype=torch.float32, device=dev)
        dc = torch.empty(L, D, dtype=torch.float32, device=dev)
        lib = _lib.lib()
        ws = _lib.workspace(lib.tzr_cross_v2_bwd_workspace(B, D, R, L), dev)
        rc = lib.tzr_cross_v2_bwd(_lib.ptr(gy), _lib.scalar_row_stride(gy), _lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr(xs), _lib.ptr(t),
                                  _lib.ptr_array(params[:L]), _lib.ptr_array(params[L:2 * L]), _lib.ptr_array(params[2 * L:]), L, B, D, R,
                                  _lib.ptr(dx), D, _lib.ptr(du), _lib.ptr(dv), _lib.ptr(dc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "tzr_cross_v2_bwd")
        return (dx, None, None, *[du[l] for l in range(L)], *[dv[l] for l in range(L)], *[dc[l] for l in range(L)])


class CrossV2(nn.Module):
    """Cross layers of Deep & Cross v2 with low-rank kernels (https://arxiv.org/pdf/2008.13535), the reference module's
    constructor, parameters, initialisation (nn.Linear's default) and forward (tzrec/modules/interaction.py:135-180):
    `u_kernels.<i>.weight` [low_rank, input_dim], `v_kernels.<i>.weight` [input_dim, low_rank], `v_kernels.<i>.bias` [input_dim]."""

    def __init__(self, input_dim: int, cross_num: int = 3, low_rank: int = 32) -> None:
        super().__init__()
        self.cross_num = cross_num
        self._low_rank = low_rank
        self._input_dim = input_dim
        self.u_kernels = nn.ModuleList([nn.Linear(input_dim, low_rank, bias=False) for _ in range(cross_num)])
        self.v_kernels = nn.ModuleList([nn.Linear(low_rank, input_dim, bias=True) for _ in range(cross_num)])

    def output_dim(self) -> int:
        return self._input_dim

    def _fused_ok(self, x: torch.Tensor) -> bool:
        return bool(FUSED_CROSS_V2 and x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] > 0 and not _traced(x)
                    and 1 <= self.cross_num <= CROSS_V2_MAX_LAYERS and 1 <= x.shape[1] <= CROSS_V2_MAX_DIM
                    and x.shape[1] == self._input_dim and 1 <= self._low_rank <= CROSS_V2_MAX_RANK
                    and self.u_kernels[0].weight.dtype == torch.float32 and (x.is_cuda or _lib.emulated()))

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if self._fused_ok(input):
            params = [m.weight for m in self.u_kernels] + [m.weight for m in self.v_kernels] + [m.bias for m in self.v_kernels]
            save = torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in params))  # (inference: nothing is kept)
            return _CrossV2Fn.apply(input, self.cross_num, save, *params)
        x_0 = x_l = input
        for i in range(self.cross_num):  # the reference's literal form
            x_l = x_0 * self.v_kernels[i](self.u_kernels[i](x_l)) + x_l
        return x_l


FUSED_CIN = True  # A/B switch: False = the reference's literal loop (einsum to [B, H F, D], Conv1d, sum per layer)
CIN_MAX_DIM, CIN_MAX_FEATURES, CIN_MAX_LAYER_SIZE, CIN_MAX_LAYERS = 64, 64, 256, 4  # CIN_MAXD, CIN_MAXF, CIN_MAXO, CIN_MAXL of csrc/cin.hip


class _CINFn(torch.autograd.Function):
    """y = cat_i sum_d X^{i+1} on tzr_cin_fwd (one launch, saves X^1 .. X^{L-1}) and tzr_cin_bwd (2 L + 1 launches), which returns
    the input gradient and every layer's finished weight and bias gradient (pieces of one buffer).  The backward writes dX^i
    over the saved X^i, so it runs once per forward."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, F: int, D: int, layers, *params: torch.Tensor):
        x = _lib.scalar_rows(x)
        B, L = x.shape[0], len(layers)
        params = tuple(p if p.is_contiguous() else p.contiguous() for p in params)
        y = torch.empty(B, sum(layers), dtype=torch.float32, device=x.device)
        save = any(ctx.needs_input_grad)
        xs = [torch.empty(B, o, D, dtype=torch.float32, device=x.device) for o in layers[:-1]] if save else []
        sizes = (C.c_int * L)(*layers)
        rc = _lib.lib().tzr_cin_fwd(_lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr_array(params[:L]), _lib.ptr_array(params[L:]), sizes, L, B, F, D,
                                    _lib.ptr_array(xs) if xs else None, _lib.ptr(y), y.shape[1], _lib.stream_ptr(x.device))
        _lib.check(rc, "tzr_cin_fwd")
        ctx.save_for_backward(x, *params[:L], *xs)
        ctx.cfg, ctx.consumed = (F, D, tuple(layers)), False
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        F, D, layers = ctx.cfg
        L = len(layers)
        x, *rest = ctx.saved_tensors
        ws_, xs = rest[:L], rest[L:]
        if ctx.consumed:
            raise RuntimeError("CIN: the backward overwrites the saved activations with their gradients and ran already; "
                               "run the forward again (or set interaction.FUSED_CIN = False) for a second backward")
        ctx.consumed = True
        B = x.shape[0]
        gy = _lib.scalar_rows(gy)
        hs = (F,) + layers[:-1]
        total = sum(o * h * F + o for o, h in zip(layers, hs))
        gx = torch.empty(B, F * D, dtype=torch.float32, device=x.device)
        dwc = torch.empty(total, dtype=torch.float32, device=x.device)
        lib, sizes = _lib.lib(), (C.c_int * L)(*layers)
        ws = _lib.workspace(lib.tzr_cin_bwd_workspace(B, F, D, sizes, L), x.device)
        rc = lib.tzr_cin_bwd(_lib.ptr(gy), _lib.scalar_row_stride(gy), _lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr_array(ws_), sizes, L, B, F, D,
                             _lib.ptr_array(xs) if xs else None, _lib.ptr(gx), F * D, _lib.ptr(dwc), _lib.ptr(ws), ws.numel(),
                             _lib.stream_ptr(x.device))
        _lib.check(rc, "tzr_cin_bwd")
        gws, gcs, off = [], [], 0
        for o, h in zip(layers, hs):
            gws.append(dwc[off:off + o * h * F].view(o, h * F, 1))
            gcs.append(dwc[off + o * h * F:off + o * h * F + o])
            off += o * h * F + o
        return (gx, None, None, None, *gws, *gcs)


class CIN(nn.Module):
    """Compressed interaction network of xDeepFM (https://arxiv.org/pdf/1803.05170), the reference module's constructor,
    parameters and forward (tzrec/modules/interaction.py:183-233): `cin_layers.<i>` is a Conv1d(H_i F, O_i, kernel_size=1)."""

    def __init__(self, feature_num: int, cin_layer_size) -> None:
        super().__init__()
        self.feature_num = feature_num
        self.cin_layer_size = list(cin_layer_size)
        self.cin_layers = nn.ModuleList()
        for i, layer_size in enumerate(self.cin_layer_size):
            in_channels = feature_num * (self.cin_layer_size[i - 1] if i > 0 else feature_num)
            self.cin_layers.append(nn.Conv1d(in_channels=in_channels, out_channels=layer_size, kernel_size=1))

    def output_dim(self) -> int:
        return sum(self.cin_layer_size)

    def _fused_ok(self, x: torch.Tensor) -> bool:
        L = len(self.cin_layer_size)
        return bool(FUSED_CIN and x.dim() == 3 and x.dtype == torch.float32 and x.shape[0] > 0 and not _traced(x)
                    and x.shape[1] == self.feature_num and 1 <= L <= CIN_MAX_LAYERS
                    and 1 <= x.shape[1] <= CIN_MAX_FEATURES and 1 <= x.shape[2] <= CIN_MAX_DIM
                    and all(1 <= o <= CIN_MAX_LAYER_SIZE for o in self.cin_layer_size)
                    and all(m.weight.dtype == torch.float32 and m.bias is not None for m in self.cin_layers)
                    and (x.is_cuda or _lib.emulated()))

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if self._fused_ok(input):
            B, F, D = input.shape
            # (a view of a group tensor, or of a column slice of one, reshapes to its [B, F D] rows as they lie: no copy)
            return _CINFn.apply(input.reshape(B, F * D), F, D, tuple(self.cin_layer_size), *[m.weight for m in self.cin_layers],
                                *[m.bias for m in self.cin_layers])
        batch_size, field_num, embed_dim = input.shape
        x_vec, x_out = input, []
        for i, o in enumerate(self.cin_layer_size):  # the reference's literal form
            z = torch.einsum("bhd,bfd->bhfd", x_vec, input)
            z = z.reshape(batch_size, field_num * (self.cin_layer_size[i - 1] if i > 0 else field_num), embed_dim)
            x_vec = self.cin_layers[i](z)
            x_out.append(torch.sum(x_vec, dim=2))
        return torch.cat(x_out, dim=1) if x_out else input.new_zeros(batch_size, 0)
