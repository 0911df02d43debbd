"""The behaviour-to-interest capsule layer of MIND (tzrec/modules/capsule.py) on jagged rows.

`capsule_routing` is the layer's forward (capsule.py:125-231) -- pad / truncate to max_seq_len, low capsules X W, num_iters rounds
of dynamic routing, squash, capsule mask -- in one autograd Function over tzr_capsule_fwd / _bwd (csrc/capsule_routing.hip): one
launch forward, two backward, nothing of shape [B, S, H] in memory.  `FUSED_CAPSULE = False`, or a shape outside `capsule_ok`,
runs `capsule_literal`, the reference's padded form word for word.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import nn

from . import _lib

FUSED_CAPSULE = True  # profiles/capsule: the fused layer against the literal one, forward + backward


@dataclass(frozen=True)
class CapsuleConfig:
    """the fields of the reference's B2ICapsule message, with its defaults (tzrec/protos/module.proto)"""
    max_k: int = 5
    max_seq_len: int = 50
    high_dim: int = 8
    num_iters: int = 3
    routing_logits_scale: float = 20.0
    routing_logits_stddev: float = 1.0
    squash_pow: float = 1.0
    const_caps_num: bool = False
    routing_init_method: str = "normal"


def squash(x: torch.Tensor, squash_pow: float) -> torch.Tensor:
    """capsule.py:105-123"""
    norm = torch.linalg.norm(x, dim=-1, keepdim=True)
    norm_eps = torch.max(norm, torch.tensor(1e-7, dtype=x.dtype, device=x.device))
    scale_factor = torch.pow(torch.square(norm_eps) / (1 + torch.square(norm_eps)), squash_pow) / norm_eps
    return scale_factor * x


def capsule_literal(x: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, cfg: CapsuleConfig,
                    logits0: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's padded form (capsule.py:125-231) on x [N, L] rows with offsets [B + 1]: -> (high [B, K, H], mask [B, K]
    bool).  logits0 [N, K]: the initial routing logits of the rows (None: zeros); a padded position's never matter, its
    weights are multiplied by the sequence mask."""
    N, L = x.shape
    S, K = cfg.max_seq_len, cfg.max_k
    dev = x.device
    seq_len = offsets[1:] - offsets[:-1]
    pos = torch.arange(S, device=dev)
    seq_mask = pos[None, :] < seq_len[:, None]  # [B, S]
    # [B, S, L]: truncated, or padded -- a padded position reads a later row (a spare zero row behind the last) and is zeroed by the
    # reference's own mask multiply; one shared padding row would take every padded position's (zero) gradient in the backward's
    # scatter, 92 ms of a pass at B = 8192 (NOTES.md)
    idx = (offsets[:-1, None] + pos[None, :]).clamp(max=N)
    seq_mask_f = seq_mask.to(x.dtype)
    inputs = torch.cat([x, x.new_zeros(1, L)], dim=0)[idx] * seq_mask_f.unsqueeze(-1)
    if cfg.const_caps_num:
        n_high = torch.zeros_like(seq_len, dtype=torch.float32) + K
    else:
        n_high = torch.maximum(torch.tensor([1.0], device=dev), torch.minimum(torch.tensor([float(K)], device=dev), torch.log2(seq_len.float())))
    capsule_mask = torch.arange(K, device=dev)[None, :] < n_high[:, None]  # [B, K]
    if logits0 is None:
        routing_logits = x.new_zeros(idx.shape + (K,))
    else:
        routing_logits = torch.cat([logits0.to(x.dtype), x.new_zeros(1, K)], dim=0)[idx]
    routing_logits = routing_logits.detach() * cfg.routing_logits_stddev
    thresh = (capsule_mask.unsqueeze(1).to(x.dtype) * 2 - 1) * float("inf")
    low = torch.einsum("bsl, lh -> bsh", inputs, weight)
    low_detach = low.detach()
    low_detach_norm = torch.nn.functional.normalize(low_detach, p=2.0, dim=-1)
    high = None
    for it in range(cfg.num_iters):
        routing_logits = torch.minimum(routing_logits, thresh)
        routing_logits = torch.nn.functional.softmax(routing_logits * cfg.routing_logits_scale, dim=2)
        routing_logits = routing_logits * seq_mask_f.unsqueeze(2)
        if it + 1 < cfg.num_iters:
            high = torch.einsum("bsh,bsk->bkh", low_detach, routing_logits)
            routing_logits = routing_logits + torch.einsum("bkh, bsh -> bsk", high, low_detach_norm)
        else:
            high = squash(torch.einsum("bsh,bsk->bkh", low, routing_logits), cfg.squash_pow)
    return high * capsule_mask.unsqueeze(-1).to(x.dtype), capsule_mask


def capsule_ok(x: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, cfg: CapsuleConfig,
               logits0: Optional[torch.Tensor] = None) -> bool:
    """what tzr_capsule_* takes: fp32 x [N, L] with unit column stride, a row stride that is a multiple of 4 floats and 16-byte
    aligned rows (a column slice of a wider buffer is fine); offsets int64 [B + 1] contiguous; weight [L, H] contiguous; logits0
    [N, K] contiguous or None; L, H multiples of 4 in [4, 128]; 1 <= K <= 8; 1 <= num_iters <= 8; 1 <= S <= 128 with
    ceil16(S) * H <= 8192; routing_logits_scale > 0; everything on the device of the loaded library"""
    if x.dim() != 2 or weight.dim() != 2 or offsets.dim() != 1 or offsets.numel() < 1:
        return False
    (N, L), H, K, S = x.shape, weight.shape[1], cfg.max_k, cfg.max_seq_len
    if not _lib.takes(x) or weight.device != x.device or offsets.device != x.device:
        return False
    if not (L % 4 == 0 and 4 <= L <= _lib.CAPSULE_MAX_DIM and H % 4 == 0 and 4 <= H <= _lib.CAPSULE_MAX_DIM and weight.shape[0] == L):
        return False
    if not (1 <= K <= _lib.CAPSULE_MAX_K and 1 <= cfg.num_iters <= _lib.CAPSULE_MAX_ITERS and 1 <= S <= _lib.CAPSULE_MAX_S
            and (S + 15) // 16 * 16 * H <= _lib.CAPSULE_MAX_SH and cfg.routing_logits_scale > 0):
        return False
    if not (_lib.packed_ok(weight, (L, H), x.device, aligned=True) and offsets.dtype == torch.int64 and offsets.is_contiguous()):
        return False
    if N > 0 and not _lib.rows_ok(x, L):
        return False
    if x.dtype != torch.float32 or N >= 2 ** 31 or offsets.numel() - 1 >= 2 ** 31:
        return False
    return logits0 is None or _lib.packed_ok(logits0, (N, K), x.device)


class _CapsuleFn(torch.autograd.Function):
    """Inputs: x [N, L], offsets [B + 1], weight [L, H], logits0 [N, K] or None.  Outputs: high [B, K, H], mask [B, K] bool, c
    [N, K] (the final routing weights); only `high` carries a gradient, to x and weight.  Saved for the backward: the inputs,
    c and the capsules in front of the squash [B, K, H].  Capturable: every buffer is torch's, nothing is read back."""

    @staticmethod
    def _fill(m, x, offsets, weight, logits0, cfg, c, pre):
        m.B, m.N, m.L, m.H = offsets.numel() - 1, x.shape[0], x.shape[1], weight.shape[1]
        m.K, m.S, m.num_iters, m.const_caps_num = cfg.max_k, cfg.max_seq_len, cfg.num_iters, int(bool(cfg.const_caps_num))
        m.scale, m.stddev, m.squash_pow = float(cfg.routing_logits_scale), float(cfg.routing_logits_stddev), float(cfg.squash_pow)
        if x.shape[0] > 0:
            m.x, m.x_stride, m.c = _lib.ptr(x), x.stride(0), _lib.ptr(c)
        else:
            m.x_stride = x.shape[1]
        m.offsets, m.w, m.pre = _lib.ptr(offsets), _lib.ptr(weight), _lib.ptr(pre)
        m.logits0 = _lib.opt_ptr(logits0) if x.shape[0] > 0 else 0

    @staticmethod
    def forward(ctx, x, offsets, weight, logits0, cfg):
        B, K, H, dev = offsets.numel() - 1, cfg.max_k, weight.shape[1], x.device
        f32 = dict(dtype=torch.float32, device=dev)
        high, pre = torch.empty(B, K, H, **f32), torch.empty(B, K, H, **f32)
        mask = torch.empty(B, K, dtype=torch.bool, device=dev)
        c = torch.empty(x.shape[0], K, **f32)
        m = _lib.TzrCapsule()
        _CapsuleFn._fill(m, x, offsets, weight, logits0, cfg, c, pre)
        m.high, m.high_stride, m.mask = _lib.ptr(high), H, _lib.ptr(mask)
        _lib.launch("tzr_capsule_fwd", m, dev)
        ctx.save_for_backward(x, offsets, weight, c, pre)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(mask, c)
        ctx.set_materialize_grads(False)  # (no zero-filled gradients for mask and c: two launches a pass)
        return high, mask, c

    @staticmethod
    def backward(ctx, ghigh, _gmask, _gc):
        if ghigh is None:
            return None, None, None, None, None
        x, offsets, weight, c, pre = ctx.saved_tensors
        cfg, dev = ctx.cfg, x.device
        g = ghigh.to(torch.float32)
        if not _lib.rows3_ok(g):
            g = g.clone(memory_format=torch.contiguous_format)  # (.contiguous() keeps the odd strides of a 1-row tensor)
        dx = torch.empty(x.shape, dtype=torch.float32, device=dev)
        dw = torch.empty(weight.shape, dtype=torch.float32, device=dev)
        m = _lib.TzrCapsule()
        _CapsuleFn._fill(m, x, offsets, weight, None, cfg, c, pre)
        m.grad_high, m.grad_high_stride, m.dw = _lib.ptr(g), g.stride(1), _lib.ptr(dw)
        if x.shape[0] > 0:
            m.dx, m.dx_stride = _lib.ptr(dx), dx.stride(0)
        else:
            m.dx_stride = x.shape[1]
        _lib.launch_ws("tzr_capsule", m, dev, "tzr_capsule_bwd")
        return dx, None, dw, None, None


def capsule_routing(x: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, cfg: CapsuleConfig,
                    logits0: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (high [B, K, H], mask [B, K] bool).  x [N, L]: the histories' rows, sample b's at offsets[b] : offsets[b + 1] (its first
    max_seq_len take part, the later ones get a zero gradient); weight [L, H]: the bilinear matrix; logits0 [N, K]: the initial
    routing logits before routing_logits_stddev (None: zeros), no gradient.  One launch forward and two backward, unless
    FUSED_CAPSULE is off or `capsule_ok` refuses the shape: then `capsule_literal` runs.  A batch without samples is the
    literal form's too."""
    if logits0 is not None:
        logits0 = logits0.detach()
    if FUSED_CAPSULE and offsets.numel() > 1 and capsule_ok(x, offsets, weight, cfg, logits0):
        high, mask, _ = _CapsuleFn.apply(x, offsets, weight, logits0, cfg)
        return high, mask
    return capsule_literal(x, offsets, weight, cfg, logits0)


class CapsuleLayer(nn.Module):
    """tzrec/modules/capsule.py: CapsuleLayer, with the reference's parameter name `bilinear_matrix` [low_dim, high_dim].
    forward(rows [N, low_dim], offsets [B + 1]) -> (interests [B, max_k, high_dim], capsule mask [B, max_k]).
    routing_init_method "normal" draws torch.randn(N, max_k) on the rows' device (capturable; the reference draws [B, S, max_k],
    the same distribution: a padded position's logits never matter), "zeros" passes none; anything else is refused, as the
    reference asserts."""

    def __init__(self, cfg: CapsuleConfig, input_dim: int, device=None) -> None:
        super().__init__()
        if cfg.routing_init_method not in ("normal", "zeros"):
            raise ValueError(f"capsule_config.routing_init_method: {cfg.routing_init_method!r} (init_method should be 'normal' or 'zeros')")
        if cfg.num_iters <= 0:
            raise ValueError("capsule_config.num_iters should be greater than 0")
        self.cfg = cfg
        self.bilinear_matrix = nn.Parameter(torch.randn(input_dim, cfg.high_dim, device=device))

    def forward(self, rows: torch.Tensor, offsets: torch.Tensor, logits0: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """logits0 [N, max_k]: the initial routing logits instead of the layer's own draw (a recorded draw of the reference)"""
        if logits0 is None and self.cfg.routing_init_method == "normal":
            logits0 = torch.randn(rows.shape[0], self.cfg.max_k, device=rows.device, dtype=rows.dtype)
        return capsule_routing(rows, offsets, self.bilinear_matrix, self.cfg, logits0)
