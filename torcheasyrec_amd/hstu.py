"""HSTU's jagged pointwise-SiLU attention and the STU layer around it (tzrec/ops/hstu_attention.py::hstu_mha,
tzrec/modules/gr/stu.py: STULayer, STUStack): the operation under hstu_match, dlrm_hstu and ultra_hstu.

`hstu_mha` runs csrc/hstu_attention.hip (tzr_hstu_attn_fwd / _bwd: one launch forward, two backward, nothing of size N x N in
memory, work following sum(n_i^2)) when FUSED_HSTU_MHA is on and `hstu_mha_ok` takes the operands; otherwise -- the switch off, a
shape outside `hstu_mha_limit`, a double backward -- the literal padded form [B, H, N, N] out of plain torch ops.  bf16 q, k, v
take csrc/hstu_attention_bf16.hip (tzr_hstu_attn_bf16_fwd / _bwd: the same launches on the bf16 MFMAs, fp32 accumulation, bf16
out and gradients) when FUSED_HSTU_MHA_BF16 is on as well; mixed dtypes and fp16 take the literal form.  Built: causal, no
attention dropout, no min_full_attn_seq_len, no attn_func (SLA), fp32 and bf16; the rest is refused by name.

`delta_hstu_mha` is the serving side (the reference's delta_hstu_mha under STULayer.cached_forward): the last `delta` rows of every
sample against the sample's cached keys and values plus the delta rows' own.  With FUSED_HSTU_DELTA on and `delta_hstu_mha_ok`
taking the operands it runs csrc/hstu_delta.hip (tzr_hstu_delta_fwd: forward only, fp32; the keys split over the waves of a
workgroup and over workgroups, the cache and the delta rows read where they lie -- the reference's concatenated full_k / full_v
are never built) or, on bf16 operands with FUSED_HSTU_DELTA_BF16 on as well, csrc/hstu_delta_bf16.hip (tzr_hstu_delta_bf16_fwd: the
same split on the bf16 MFMAs, fp32 accumulation, bf16 out -- a stack cast to bf16 keeps a bf16 cache and serves from it);
otherwise -- mixed dtypes and fp16 too -- `delta_hstu_mha_literal`, the padded torch form.  STULayer.forward with `kv_caching_lengths` fills the
layer's cache (prefill), STULayer / STUStack.cached_forward score new rows against it.

`stu_output` is the layer's stage behind the attention (the reference's hstu_compute_output): silu(u), the layer or group norm of
the attention's rows, their product, the concat [u, attn, y], dropout and addmm(x, ., `_output_weight`) on csrc/stu_output.hip
(tzr_stu_output_fwd / _bwd: one launch forward, two backward and a finishing one; the concat, the normed rows and the dropout
mask are never in memory, the mask follows the counter rule of include/tzrec_hip.h from a seed on the device) when
FUSED_STU_OUTPUT is on and `stu_output_ok` takes the operands; otherwise `stu_output_literal`, the torch ops.  What stays torch ops
in the layer: the input norm and the uvqk product in front of the attention.

`add_positional_embeddings`, `add_timestamp_positional_embeddings` and `HSTUPositionalEncoder` are the encoder in front of the stack
(tzrec/ops/position.py, tzrec/modules/gr/positional_encoder.py): alpha x plus a row of the position table and, in the timestamp
form, a row of the time-bucket table, on the jagged rows.  With FUSED_HSTU_POSITION on and `hstu_position_ok` taking the operands
they run csrc/hstu_position.hip (tzr_hstu_pos_fwd / _bwd, fp32 and bf16: one launch forward; backward dx and the two table
gradients as fixed-order sums, no atomics, the rows' int32 buckets the only thing saved beside the integer inputs); otherwise
-- mixed dtypes, fp16, a shape outside `hstu_position_limit`, a double backward -- the literal padded form out of torch ops."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

FUSED_STU_OUTPUT = False  # profiles/stu_output, forward + backward: 6.20 ms fused against 2.84 ms literal (0.56 against 0.94 GB): the literal form stays
FUSED_HSTU_MHA = True  # profiles/hstu_attention, forward + backward: 24.4 ms fused against 32.4 ms literal, 0.72 against 14.06 GB
FUSED_HSTU_MHA_BF16 = True  # bf16 q, k, v on csrc/hstu_attention_bf16.hip (needs FUSED_HSTU_MHA too); profiles/hstu_attention_bf16
FUSED_HSTU_DELTA = True  # profiles/hstu_delta, one serving step: 95.1 us fused (94.6 - 100.9) against 646.7 us literal (644.3 - 703.2), 9.4 against 249.5 MB
# bf16 operands on csrc/hstu_delta_bf16.hip (needs FUSED_HSTU_DELTA too); profiles/hstu_delta_bf16, the same step: 54.7 us fused (54.5 - 63.5)
# against 634.7 us for the literal form in bf16 (618.4 - 697.2) and 102.3 us for the fp32 kernel, 9.2 against 127.0 MB
FUSED_HSTU_DELTA_BF16 = True
# profiles/hstu_position, forward + backward at 38 866 rows, E = 512: fp32 203.2 us fused (201.1 - 538.7) against 25.7 ms literal (25.5 - 26.8),
# 263 against 485 MB; bf16 166.5 us fused (164.4 - 169.3) against 50.3 ms literal (49.6 - 54.6), 173 against 243 MB: on for both dtypes
FUSED_HSTU_POSITION = True


def hstu_valid_mask(n: torch.Tensor, N: int, num_targets: Optional[torch.Tensor], max_attn_len: int, contextual_seq_len: int,
                    rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """_get_valid_attn_mask (tzrec/ops/_pytorch/pt_hstu_attention.py) with causal=True on the rows each sample keeps: n [B] -> bool
    [B, N, N]; with `rows` [B, R] (query positions in [0, N)) only those query rows: bool [B, R, N]"""
    ids = torch.arange(N, device=n.device).view(1, N)
    max_ids = n.view(-1, 1)
    if contextual_seq_len > 0:
        ids = torch.clamp(ids - contextual_seq_len + 1, min=0)
        max_ids = max_ids - contextual_seq_len + 1
    if num_targets is not None:
        max_ids = max_ids - num_targets.view(-1, 1)
        ids = torch.minimum(ids, max_ids)
    ids = ids.expand(n.numel(), N)
    col, max_ids = ids.unsqueeze(1), max_ids.unsqueeze(2)
    if rows is None:
        row, eye = ids.unsqueeze(2), torch.eye(N, device=n.device, dtype=torch.bool).unsqueeze(0)
    else:
        row, eye = ids.gather(1, rows).unsqueeze(2), rows.unsqueeze(2) == torch.arange(N, device=n.device).view(1, 1, N)
    dist = row - col
    valid = eye | (dist > 0)
    if max_attn_len > 0:
        valid = valid & (dist <= max_attn_len)
    if contextual_seq_len > 0:
        valid = valid | ((row == 0) & (col < max_ids))
    return valid


def hstu_mha_literal(max_seq_len: int, alpha: float, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_offsets: torch.Tensor,
                     num_targets: Optional[torch.Tensor] = None, max_attn_len: int = 0, contextual_seq_len: int = 0,
                     scaling_seqlen: int = -1) -> torch.Tensor:
    """The reference's padded form (pytorch_hstu_mha) out of plain torch ops: pads to [B, H, N, .], builds the [B, H, N, N] scores.
    A sample keeps its first max_seq_len rows; the rows behind them get zero output."""
    L, H, _ = q.shape
    N, B = int(max_seq_len), seq_offsets.numel() - 1
    scale = float(scaling_seqlen if scaling_seqlen > 0 else max_seq_len)
    n = torch.clamp(seq_offsets[1:] - seq_offsets[:-1], max=N)
    pos = torch.arange(N, device=q.device).view(1, N)
    keep = pos < n.view(-1, 1)
    # a position a sample does not have reads a later row (wrapping over a spare zero row behind the last) and is zeroed by `keep`:
    # one shared padding row would take every padded position's (zero) gradient in the gather's backward, a scatter that
    # serialises on the one row -- 62 of 94 ms of a pass at the profile's shape (NOTES.md; capsule_literal pads the same way)
    idx = (seq_offsets[:-1].view(-1, 1) + pos) % (L + 1)

    def pad(x):  # [L, H, D] -> [B, H, N, D], zeros for the rows a sample does not have
        rows = torch.cat([x.reshape(L, -1), x.new_zeros(1, x.shape[1] * x.shape[2])])[idx]
        return torch.where(keep.unsqueeze(2), rows, rows.new_zeros(())).view(B, N, H, x.shape[2]).transpose(1, 2)

    qk = F.silu(torch.einsum("bhxa,bhya->bhxy", pad(q), pad(k)) * alpha) / scale
    qk = qk * hstu_valid_mask(n, N, num_targets, max_attn_len, contextual_seq_len).unsqueeze(1)
    dense = torch.einsum("bhxy,bhyv->bhxv", qk, pad(v)).transpose(1, 2)  # [B, N, H, V]
    return v.new_zeros(L, H, v.shape[2]).index_put((idx[keep],), dense[keep])


def hstu_mha_limit(H: int, Da: int, Dv: int, max_seq_len: int, max_attn_len: int = 0, contextual_seq_len: int = 0, B: int = 1,
                   dtype: torch.dtype = torch.float32) -> Optional[str]:
    """None when tzr_hstu_attn_* (fp32) or tzr_hstu_attn_bf16_* (bf16) has a kernel for the shape, else the limit of
    csrc/hstu_attention.hip / hstu_attention_bf16.hip it misses (include/tzrec_hip.h)"""
    D, S = _lib.HSTU_MAX_DIM, _lib.HSTU_MAX_SEQ_LEN
    if dtype not in (torch.float32, torch.bfloat16):
        return f"dtype {dtype} must be float32 or bfloat16"
    step = 8 if dtype == torch.bfloat16 else 4  # (16 bytes of a row)
    for name, d in (("attention_dim", Da), ("hidden_dim", Dv)):
        if d % step or not step <= d <= D:
            return f"{name} {d} must be a multiple of {step} in [{step}, {D}]"
    if H < 1:
        return f"num_heads {H} must be at least 1"
    if not 1 <= max_seq_len <= S:
        return f"max_seq_len {max_seq_len} must be in [1, {S}]"
    if not 0 <= max_attn_len <= S:
        return f"max_attn_len {max_attn_len} must be in [0, {S}]"
    if not 0 <= contextual_seq_len <= S:
        return f"contextual_seq_len {contextual_seq_len} must be in [0, {S}]"
    block = _lib.HSTU_BF16_BLOCK if dtype == torch.bfloat16 else _lib.HSTU_BLOCK
    if (max_seq_len + block - 1) // block * max(B, 1) * H >= 2 ** 31:
        return f"grid: ceil({max_seq_len} / {block}) x {B} x {H} workgroups must stay below 2^31"
    return None


def hstu_mha_ok(max_seq_len: int, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_offsets: torch.Tensor,
                num_targets: Optional[torch.Tensor] = None, max_attn_len: int = 0, contextual_seq_len: int = 0) -> bool:
    """what tzr_hstu_attn_* / tzr_hstu_attn_bf16_* takes: q, k [L, H, Da], v [L, H, Dv] of ONE dtype, fp32 as `_lib.heads_ok`
    operands or bf16 as `_lib.heads_bf16_ok` operands (column slices of one uvqk matrix are fine), offsets int64 [B + 1] and
    num_targets int64 [B] contiguous, a shape inside `hstu_mha_limit` for that dtype, everything on the device of the loaded library"""
    if q.dim() != 3 or k.shape != q.shape or v.dim() != 3 or v.shape[:2] != q.shape[:2] or seq_offsets.dim() != 1 or seq_offsets.numel() < 1:
        return False
    dev, (L, H, Da), B = q.device, q.shape, seq_offsets.numel() - 1
    if not _lib.takes(q) or any(t.device != dev for t in (k, v, seq_offsets)) or L >= 2 ** 31 or k.dtype != q.dtype or v.dtype != q.dtype:
        return False
    if hstu_mha_limit(H, Da, v.shape[2], max_seq_len, max_attn_len, contextual_seq_len, B, q.dtype) is not None or (B == 0 and L > 0):
        return False  # (no sample, yet rows: the entry points launch nothing, so nobody would write the rows)
    if seq_offsets.dtype != torch.int64 or not seq_offsets.is_contiguous():
        return False
    if num_targets is not None and not (num_targets.shape == (B,) and num_targets.dtype == torch.int64 and num_targets.is_contiguous() and num_targets.device == dev):
        return False
    return L == 0 or all(_heads_ok(t) for t in (q, k, v))


def _heads_ok(t: torch.Tensor) -> bool:
    return _lib.heads_bf16_ok(t) if t.dtype == torch.bfloat16 else _lib.heads_ok(t)


def _entry(name: str, dtype: torch.dtype) -> str:
    """the entry point of the operands' dtype: tzr_hstu_attn_<name> or tzr_hstu_attn_bf16_<name>"""
    return f"tzr_hstu_attn_bf16_{name}" if dtype == torch.bfloat16 else f"tzr_hstu_attn_{name}"


def _fill(m, max_seq_len, alpha, q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len, scaling_seqlen):
    m.B, m.N, m.H, m.Da, m.Dv = seq_offsets.numel() - 1, q.shape[0], q.shape[1], q.shape[2], v.shape[2]
    m.max_seq_len, m.max_attn_len, m.contextual_seq_len, m.scaling_seqlen, m.alpha = max_seq_len, max_attn_len, contextual_seq_len, scaling_seqlen, alpha
    m.offsets, m.num_targets = _lib.ptr(seq_offsets), _lib.opt_ptr(num_targets)
    _operands(m, q=q, k=k, v=v)


def _operands(m, **tensors):
    for name, t in tensors.items():
        if t.shape[0] > 0:
            setattr(m, name, _lib.ptr(t))
        setattr(m, name + "_stride", t.stride(0) if t.shape[0] > 1 else max(t.stride(0), (t.shape[1] - 1) * t.stride(1) + t.shape[2]))
        setattr(m, name + "_head_stride", t.stride(1) if t.shape[1] > 1 else max(t.stride(1), t.shape[2]))


def hstu_attn_fwd(max_seq_len, alpha, q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len, scaling_seqlen) -> torch.Tensor:
    """tzr_hstu_attn_fwd on operands `hstu_mha_ok` took -> out [L, H, Dv] (torch.empty: the kernel writes every row)"""
    out = torch.empty(q.shape[0], q.shape[1], v.shape[2], dtype=q.dtype, device=q.device)
    m = _lib.TzrHstuAttn()
    _fill(m, max_seq_len, alpha, q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len, scaling_seqlen)
    _operands(m, out=out)
    _lib.launch(_entry("fwd", q.dtype), m, q.device)
    return out


def hstu_attn_bwd(gout, max_seq_len, alpha, q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len,
                  scaling_seqlen) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """tzr_hstu_attn_bwd -> dq, dk, dv: column slices of ONE [L, H (2 Da + Dv)] buffer, every row written by the kernels"""
    (L, H, Da), Dv = q.shape, v.shape[2]
    g = gout.to(q.dtype)
    if L > 0 and not _heads_ok(g):
        g = g.clone(memory_format=torch.contiguous_format)  # (.contiguous() keeps the odd strides of a one-row gradient: _lib.rows16)
    buf = torch.empty(L, H * (2 * Da + Dv), dtype=q.dtype, device=q.device)
    dq, dk, dv = (t.view(L, H, d) for t, d in zip(torch.split(buf, [H * Da, H * Da, H * Dv], dim=1), (Da, Da, Dv)))
    m = _lib.TzrHstuAttn()
    _fill(m, max_seq_len, alpha, q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len, scaling_seqlen)
    _operands(m, grad_out=g, dq=dq, dk=dk, dv=dv)
    _lib.launch(_entry("bwd", q.dtype), m, q.device)
    return dq, dk, dv


class _HstuMhaFn(torch.autograd.Function):
    """Saved for the backward: the inputs alone -- the backward recomputes every score tile.  Capturable: every buffer is torch's,
    nothing is read back.  Differentiable once (`hstu_mha(.., double_backward=True)` takes the literal form)."""

    calls = 0  # forwards that took the kernel (tests)

    @staticmethod
    def forward(ctx, q, k, v, seq_offsets, num_targets, cfg):
        _HstuMhaFn.calls += 1
        max_seq_len, alpha, rest = cfg[0], cfg[1], cfg[2:]
        ctx.save_for_backward(q, k, v, seq_offsets, num_targets)
        ctx.cfg = cfg
        return hstu_attn_fwd(max_seq_len, alpha, q.detach(), k.detach(), v.detach(), seq_offsets, num_targets, *rest)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        q, k, v, seq_offsets, num_targets = ctx.saved_tensors
        dq, dk, dv = hstu_attn_bwd(gout, ctx.cfg[0], ctx.cfg[1], q, k, v, seq_offsets, num_targets, *ctx.cfg[2:])
        return dq, dk, dv, None, None, None


def hstu_mha(max_seq_len: int, alpha: float, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_offsets: torch.Tensor,
             causal: bool = True, dropout_pr: float = 0.0, training: bool = True, num_targets: Optional[torch.Tensor] = None,
             max_attn_len: int = 0, contextual_seq_len: int = 0, min_full_attn_seq_len: int = 0, sort_by_length: bool = False,
             attn_func: Optional[torch.Tensor] = None, scaling_seqlen: int = -1, double_backward: bool = False) -> torch.Tensor:
    """The reference's hstu_mha: q, k [L, H, Da], v [L, H, Dv] jagged by seq_offsets [B + 1] -> [L, H, Dv].  `sort_by_length`
    changes no result (the kernels issue the long blocks first themselves)."""
    if not causal:
        raise NotImplementedError("hstu_mha: causal=False is not built")
    if dropout_pr > 0.0:
        raise NotImplementedError("hstu_mha: dropout_pr > 0 (attention dropout) is not built")
    if min_full_attn_seq_len > 0:
        raise NotImplementedError("hstu_mha: min_full_attn_seq_len > 0 is not built")
    if attn_func is not None:
        raise NotImplementedError("hstu_mha: attn_func (SLA / NFUNC masks) is not built")
    max_seq_len, max_attn_len, contextual_seq_len, scaling_seqlen = int(max_seq_len), int(max_attn_len), int(contextual_seq_len), int(scaling_seqlen)
    if FUSED_HSTU_MHA and not double_backward and (q.is_cuda or _lib.emulated()) and \
            (q.dtype == torch.float32 or (q.dtype == torch.bfloat16 and FUSED_HSTU_MHA_BF16)) and \
            hstu_mha_ok(max_seq_len, q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len):
        return _HstuMhaFn.apply(q, k, v, seq_offsets, num_targets, (max_seq_len, float(alpha), max_attn_len, contextual_seq_len, scaling_seqlen))
    return hstu_mha_literal(max_seq_len, alpha, q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len, scaling_seqlen)


def concat_cache_delta(cache: torch.Tensor, delta_rows: torch.Tensor, cache_offsets: torch.Tensor, delta: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's concat_2D_jagged of the cached rows (jagged by cache_offsets [B + 1]; rows behind offsets[B] are spare) with
    `delta` dense rows a sample -> (full rows [cache rows + B delta, ..], their offsets).  Plain torch ops, nothing read back."""
    B, Lc, dev = cache_offsets.numel() - 1, cache.shape[0], cache.device
    full_offsets = cache_offsets + delta * torch.arange(B + 1, device=dev)
    pos = torch.arange(Lc + delta_rows.shape[0], device=dev)
    b = torch.bucketize(pos, full_offsets[1:], right=True).clamp(max=max(B - 1, 0))
    pos = pos - full_offsets[b]
    n1 = (cache_offsets[1:] - cache_offsets[:-1])[b]
    src = torch.where(pos < n1, cache_offsets[b] + pos, Lc + b * delta + (pos - n1).clamp(max=delta - 1))  # (spare rows: some delta row)
    return torch.cat([cache, delta_rows])[src], full_offsets


def delta_hstu_mha_literal(max_seq_len: int, alpha: float, delta_q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_offsets: torch.Tensor,
                           num_targets: Optional[torch.Tensor] = None, max_attn_len: int = 0, contextual_seq_len: int = 0,
                           scaling_seqlen: int = -1, delta_k: Optional[torch.Tensor] = None, delta_v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's padded form (pytorch_cached_hstu_mha) out of plain torch ops; in the two-segment form it concatenates the
    cached and the delta rows first.  A sample whose n is above max_seq_len or below delta gets zero rows.  Operands of mixed
    dtypes (a bf16 delta_q on an fp32 cache) are promoted to their common dtype first."""
    (Ld, H, Da), Dv = delta_q.shape, v.shape[2]
    common = v.dtype
    for t in (delta_q, k, delta_k, delta_v):
        common = common if t is None else torch.promote_types(common, t.dtype)
    delta_q, k, v, delta_k, delta_v = (t if t is None or t.dtype == common else t.to(common) for t in (delta_q, k, v, delta_k, delta_v))
    N, B = int(max_seq_len), seq_offsets.numel() - 1
    if B == 0 or Ld == 0:
        return v.new_zeros(Ld, H, Dv)
    delta = Ld // B
    if delta_k is not None:
        cache_offsets = seq_offsets
        k, seq_offsets = concat_cache_delta(k.reshape(k.shape[0], H * Da), delta_k.reshape(Ld, H * Da), cache_offsets, delta)
        v, _ = concat_cache_delta(v.reshape(v.shape[0], H * Dv), delta_v.reshape(Ld, H * Dv), cache_offsets, delta)
    L = k.shape[0]
    scale = float(scaling_seqlen if scaling_seqlen > 0 else max_seq_len)
    n = seq_offsets[1:] - seq_offsets[:-1]
    n = torch.where((n <= N) & (n >= delta), n, torch.zeros_like(n))  # (a refused sample keeps no key: zero rows)
    pos = torch.arange(N, device=k.device).view(1, N)
    keep = pos < n.view(-1, 1)
    idx = (seq_offsets[:-1].view(-1, 1) + pos) % (L + 1)  # (padding as hstu_mha_literal)

    def pad(x, D):  # [L, H D] -> [B, H, N, D], zeros for the rows a sample does not have
        rows = torch.cat([x.reshape(L, H * D), x.new_zeros(1, H * D)])[idx]
        return torch.where(keep.unsqueeze(2), rows, rows.new_zeros(())).view(B, N, H, D).transpose(1, 2)

    rows =((n - delta).clamp(min=0).view(-1, 1) + torch.arange(delta, device=k.device).view(1, -1)).clamp(max=N - 1)  # the delta rows' positions
    qk = F.silu(torch.einsum("bhxa,bhya->bhxy", delta_q.reshape(B, delta, H, Da).transpose(1, 2), pad(k, Da)) * alpha) / scale
    qk = qk * hstu_valid_mask(n, N, num_targets, max_attn_len, contextual_seq_len, rows).unsqueeze(1)
    return torch.einsum("bhxy,bhyv->bhxv", qk, pad(v, Dv)).transpose(1, 2).reshape(Ld, H, Dv)


def delta_hstu_mha_limit(H: int, Da: int, Dv: int, max_seq_len: int, delta: int, max_attn_len: int = 0, contextual_seq_len: int = 0,
                         B: int = 1, dtype: torch.dtype = torch.float32) -> Optional[str]:
    """None when tzr_hstu_delta_fwd (fp32) or tzr_hstu_delta_bf16_fwd (bf16) has a kernel for the shape, else the limit of
    csrc/hstu_delta.hip / hstu_delta_bf16.hip it misses (include/tzrec_hip.h): the widths go in steps of 4 (fp32) or 8 (bf16)"""
    word = hstu_mha_limit(H, Da, Dv, max_seq_len, max_attn_len, contextual_seq_len, 1, dtype)
    if word is not None:
        return word
    if delta < 1:
        return f"delta {delta} must be at least 1"
    if max(B, 1) * delta * H >= 2 ** 31:
        return f"rows: {B} x {delta} x {H} must stay below 2^31"
    chunks = (max_seq_len + _lib.HSTU_DELTA_CHUNK - 1) // _lib.HSTU_DELTA_CHUNK
    if chunks * ((delta + 15) // 16) * max(B, 1) * H >= 2 ** 31:
        return f"grid: {chunks} x ceil({delta} / 16) x {B} x {H} workgroups must stay below 2^31"
    return None


def delta_hstu_mha_ok(max_seq_len: int, delta_q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_offsets: torch.Tensor,
                      num_targets: Optional[torch.Tensor] = None, max_attn_len: int = 0, contextual_seq_len: int = 0,
                      delta_k: Optional[torch.Tensor] = None, delta_v: Optional[torch.Tensor] = None) -> bool:
    """what tzr_hstu_delta_fwd / tzr_hstu_delta_bf16_fwd takes: delta_q [B delta, H, Da], k [Nc, H, Da], v [Nc, H, Dv] and, both or
    neither, delta_k [B delta, H, Da], delta_v [B delta, H, Dv], all of ONE dtype, fp32 as `_lib.heads_ok` operands or bf16 as
    `_lib.heads_bf16_ok` operands (column slices of a uvqk matrix are fine), offsets int64 [B + 1] and num_targets int64 [B]
    contiguous, a shape inside `delta_hstu_mha_limit` for that dtype, everything on the device of the loaded library"""
    if delta_q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or k.shape[1:] != delta_q.shape[1:] or v.shape[:2] != k.shape[:2] or seq_offsets.dim() != 1:
        return False
    dev, (Ld, H, Da), Dv, B = delta_q.device, delta_q.shape, v.shape[2], seq_offsets.numel() - 1
    if (delta_k is None) != (delta_v is None) or B < 0 or (B == 0 and Ld > 0) or (B > 0 and (Ld == 0 or Ld % B)):
        return False  # (no sample, yet rows: the entry point launches nothing, so nobody would write the rows)
    rest = [t for t in (k, v, delta_k, delta_v) if t is not None]
    dtype = delta_q.dtype
    if not _lib.takes(delta_q) or dtype not in (torch.float32, torch.bfloat16) or any(t.device != dev or t.dtype != dtype for t in rest) or \
            seq_offsets.device != dev or k.shape[0] >= 2 ** 31:
        return False
    if delta_k is not None and (delta_k.shape != delta_q.shape or delta_v.shape != (Ld, H, Dv)):
        return False
    if delta_hstu_mha_limit(H, Da, Dv, max_seq_len, Ld // B if B else 1, max_attn_len, contextual_seq_len, B, dtype) is not None:
        return False
    if seq_offsets.dtype != torch.int64 or not seq_offsets.is_contiguous():
        return False
    if num_targets is not None and not (num_targets.shape == (B,) and num_targets.dtype == torch.int64 and num_targets.is_contiguous() and num_targets.device == dev):
        return False
    return all(t.shape[0] == 0 or _heads_ok(t) for t in (delta_q, *rest))


class _HstuDeltaFn:
    """tzr_hstu_delta_fwd, or tzr_hstu_delta_bf16_fwd for bf16, on operands `delta_hstu_mha_ok` took -> out in their dtype.  Forward
    only: no autograd node (an input that needs a gradient takes the literal form).  Capturable: every buffer is torch's, the workspace included; nothing is read back."""

    calls = 0  # calls that took the kernel (tests)

    @staticmethod
    def apply(delta_q, k, v, seq_offsets, num_targets, delta_k, delta_v, cfg) -> torch.Tensor:
        _HstuDeltaFn.calls += 1
        max_seq_len, alpha, max_attn_len, contextual_seq_len, scaling_seqlen = cfg
        (Ld, H, Da), Dv, B = delta_q.shape, v.shape[2], seq_offsets.numel() - 1
        out = torch.empty(Ld, H, Dv, dtype=delta_q.dtype, device=delta_q.device)  # (the kernels write every row)
        if B == 0:
            return out
        m = _lib.TzrHstuDelta()
        m.B, m.Nc, m.H, m.Da, m.Dv, m.delta = B, k.shape[0], H, Da, Dv, Ld // B
        m.max_seq_len, m.max_attn_len, m.contextual_seq_len, m.scaling_seqlen, m.alpha = max_seq_len, max_attn_len, contextual_seq_len, scaling_seqlen, alpha
        m.offsets, m.num_targets = _lib.ptr(seq_offsets), _lib.opt_ptr(num_targets)
        _operands(m, delta_q=delta_q.detach(), k=k.detach(), v=v.detach(), out=out)
        if delta_k is not None:
            _operands(m, k_delta=delta_k.detach(), v_delta=delta_v.detach())
        # (one workspace symbol for both entries: the chunks' partials are fp32 either way)
        _lib.launch_ws("tzr_hstu_delta", m, delta_q.device, "tzr_hstu_delta_bf16_fwd" if delta_q.dtype == torch.bfloat16 else "tzr_hstu_delta_fwd")
        return out


def delta_hstu_mha(max_seq_len: int, alpha: float, delta_q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_offsets: torch.Tensor,
                   num_targets: Optional[torch.Tensor] = None, max_attn_len: int = 0, contextual_seq_len: int = 0, scaling_seqlen: int = -1,
                   delta_k: Optional[torch.Tensor] = None, delta_v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's delta_hstu_mha: the last delta = delta_q.shape[0] // B rows of every sample as queries [B delta, H, Da] against
    the sample's whole sequence -> [B delta, H, Dv].  Without delta_k / delta_v, k [L, H, Da], v [L, H, Dv] and seq_offsets are the
    FULL sequences (the reference's meaning: their last delta rows are the delta keys).  With them, k, v, seq_offsets are the cached
    rows alone and delta_k [B delta, H, Da], delta_v [B delta, H, Dv] follow them: the kernel reads both segments where they lie.
    max_seq_len counts cache + delta in both forms; a sample above it (or, in the one-segment form, shorter than delta) gets zero
    rows.  The kernels (csrc/hstu_delta.hip for fp32, csrc/hstu_delta_bf16.hip for bf16 with FUSED_HSTU_DELTA_BF16 on as well) are
    forward only: with FUSED_HSTU_DELTA off, an input that needs a gradient, mixed dtypes, a dtype other than fp32 and bf16 or a
    shape outside `delta_hstu_mha_limit`, the literal form runs."""
    max_seq_len, max_attn_len, contextual_seq_len, scaling_seqlen = int(max_seq_len), int(max_attn_len), int(contextual_seq_len), int(scaling_seqlen)
    given = [t for t in (delta_q, k, v, delta_k, delta_v) if t is not None]
    if FUSED_HSTU_DELTA and (delta_q.is_cuda or _lib.emulated()) and \
            (delta_q.dtype == torch.float32 or (delta_q.dtype == torch.bfloat16 and FUSED_HSTU_DELTA_BF16)) and \
            not (torch.is_grad_enabled() and any(t.requires_grad for t in given)) and \
            delta_hstu_mha_ok(max_seq_len, delta_q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len, delta_k, delta_v):
        return _HstuDeltaFn.apply(delta_q, k, v, seq_offsets, num_targets, delta_k, delta_v,
                                  (max_seq_len, float(alpha), max_attn_len, contextual_seq_len, scaling_seqlen))
    return delta_hstu_mha_literal(max_seq_len, alpha, delta_q, k, v, seq_offsets, num_targets, max_attn_len, contextual_seq_len,
                                  scaling_seqlen, delta_k, delta_v)


def stu_output_literal(u: torch.Tensor, attn: torch.Tensor, x: torch.Tensor, norm_weight: torch.Tensor, norm_bias: torch.Tensor,
                       output_weight: torch.Tensor, num_heads: int, group_norm: bool, dropout_ratio: float, training: bool,
                       eps: float = 1e-6) -> torch.Tensor:
    """the stage out of plain torch ops, on the RAW u slice (silu not yet applied)"""
    u, L, H = F.silu(u), x.shape[0], num_heads
    Dv = attn.shape[1] // H
    if group_norm:
        y = u * F.group_norm(attn.view(L, H, Dv), H, norm_weight, norm_bias, eps).view(L, H * Dv)
    else:
        y = u * F.layer_norm(attn, (H * Dv,), norm_weight, norm_bias, eps)
    y = F.dropout(torch.cat([u, attn, y], dim=1), p=dropout_ratio, training=training)
    return torch.addmm(x, y, output_weight)


def stu_output_limit(E: int, H: int, Dv: int, group_norm: bool) -> Optional[str]:
    """None when tzr_stu_output_* has a kernel for the shape, else the limit of csrc/stu_output.hip it misses (include/tzrec_hip.h)"""
    D = _lib.STU_OUT_MAX_DIM
    if H < 1 or Dv < 1:
        return f"num_heads {H} and hidden_dim {Dv} must be at least 1"
    if E % 4 or not 4 <= E <= D:
        return f"embedding_dim {E} must be a multiple of 4 in [4, {D}]"
    if (H * Dv) % 4 or not 4 <= H * Dv <= D:
        return f"num_heads x hidden_dim {H * Dv} must be a multiple of 4 in [4, {D}]"
    if group_norm and Dv % 4:
        return f"hidden_dim {Dv} must be a multiple of 4 under group norm"
    return None


def stu_output_ok(u: torch.Tensor, attn: torch.Tensor, x: torch.Tensor, norm_weight: torch.Tensor, norm_bias: torch.Tensor,
                  output_weight: torch.Tensor, num_heads: int, group_norm: bool, dropout_ratio: float = 0.0) -> bool:
    """what tzr_stu_output_* takes: u, attn [L, W] and x [L, E] as `_lib.rows_ok` operands (u a column slice of the uvqk matrix),
    the norm's pair [W] or [H] and the weight [3 W, E] contiguous fp32, a shape inside `stu_output_limit`, 0 <= p < 1, everything
    on the device of the loaded library"""
    if u.dim() != 2 or attn.shape != u.shape or x.dim() != 2 or x.shape[0] != u.shape[0] or num_heads < 1 or u.shape[1] % num_heads:
        return False
    dev, (L, W), E, H = x.device, u.shape, x.shape[1], num_heads
    if not _lib.takes(x) or any(t.device != dev for t in (u, attn)) or L >= 2 ** 31 or not 0.0 <= dropout_ratio < 1.0:
        return False
    if stu_output_limit(E, H, W // H, group_norm) is not None:
        return False
    n = (H,) if group_norm else (W,)
    if not (_lib.packed_ok(norm_weight, n, dev, True) and _lib.packed_ok(norm_bias, n, dev, True) and _lib.packed_ok(output_weight, (3 * W, E), dev, True)):
        return False
    return L == 0 or (_lib.rows_ok(u) and _lib.rows_ok(attn) and _lib.rows_ok(x))


def _stu_fill(m, u, attn, norm_weight, norm_bias, output_weight, seed, mean, rstd, cfg):
    H, group_norm, p, training, eps = cfg
    m.L, m.E, m.H, m.Dv = u.shape[0], output_weight.shape[1], H, u.shape[1] // H
    m.group_norm, m.training, m.eps, m.p = int(group_norm), int(training), eps, p
    m.u, m.u_stride, m.attn, m.attn_stride = _lib.ptr(u), _lib.scalar_row_stride(u), _lib.ptr(attn), _lib.scalar_row_stride(attn)
    m.gamma, m.beta, m.wo, m.seed = _lib.ptr(norm_weight), _lib.ptr(norm_bias), _lib.ptr(output_weight), _lib.opt_ptr(seed)
    m.mean, m.rstd = _lib.ptr(mean), _lib.ptr(rstd)


def stu_output_fwd(u, attn, x, norm_weight, norm_bias, output_weight, seed, cfg) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """tzr_stu_output_fwd on operands `stu_output_ok` took -> out [L, E], mean, rstd [L] or [L, H] (the kernel writes every row)"""
    L, groups = u.shape[0], cfg[0] if cfg[1] else 1
    out = torch.empty(L, x.shape[1], dtype=torch.float32, device=x.device)
    mean, rstd = torch.empty(L, groups, dtype=torch.float32, device=x.device), torch.empty(L, groups, dtype=torch.float32, device=x.device)
    if L > 0:
        m = _lib.TzrStuOutput()
        _stu_fill(m, u, attn, norm_weight, norm_bias, output_weight, seed, mean, rstd, cfg)
        m.x, m.x_stride, m.out, m.out_stride = _lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr(out), out.shape[1]
        _lib.launch("tzr_stu_output_fwd", m, x.device)
    return out, mean, rstd


def stu_output_bwd(gout, u, attn, norm_weight, norm_bias, output_weight, seed, mean, rstd, cfg):
    """tzr_stu_output_bwd -> du, dattn [L, W], dWo [3 W, E], dgamma, dbeta; every element written by the kernels (zeros at L == 0)"""
    (L, W), E, dev = u.shape, output_weight.shape[1], u.device
    if L == 0:
        return u.new_zeros(0, W), u.new_zeros(0, W), torch.zeros_like(output_weight), torch.zeros_like(norm_weight), torch.zeros_like(norm_bias)
    g = _lib.rows16(gout.to(torch.float32))
    du, dattn = torch.empty(L, W, dtype=torch.float32, device=dev), torch.empty(L, W, dtype=torch.float32, device=dev)
    dwo, dgamma, dbeta = torch.empty_like(output_weight), torch.empty_like(norm_weight), torch.empty_like(norm_bias)
    m = _lib.TzrStuOutput()
    _stu_fill(m, u, attn, norm_weight, norm_bias, output_weight, seed, mean, rstd, cfg)
    m.grad_out, m.grad_out_stride = _lib.ptr(g), _lib.scalar_row_stride(g)
    m.du, m.du_stride, m.dattn, m.dattn_stride = _lib.ptr(du), W, _lib.ptr(dattn), W
    m.dwo, m.dgamma, m.dbeta = _lib.ptr(dwo), _lib.ptr(dgamma), _lib.ptr(dbeta)
    _lib.launch_ws("tzr_stu_output_bwd", m, dev, "tzr_stu_output_bwd")
    return du, dattn, dwo, dgamma, dbeta


class _StuOutputFn(torch.autograd.Function):
    """Saved for the backward: the inputs, mean, rstd and the seed tensor -- nothing of width 3 W, no mask.  Capturable: every
    buffer is torch's, the seed stays on the device.  Differentiable once (`stu_output(.., double_backward=True)` takes the
    literal form)."""

    calls = 0  # forwards that took the kernel (tests)

    @staticmethod
    def forward(ctx, u, attn, x, norm_weight, norm_bias, output_weight, seed, cfg):
        _StuOutputFn.calls += 1
        out, mean, rstd = stu_output_fwd(u.detach(), attn.detach(), x.detach(), norm_weight.detach(), norm_bias.detach(), output_weight.detach(), seed, cfg)
        ctx.save_for_backward(u, attn, norm_weight, norm_bias, output_weight, seed, mean, rstd)
        ctx.cfg = cfg
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        du, dattn, dwo, dgamma, dbeta = stu_output_bwd(gout, *ctx.saved_tensors, ctx.cfg)
        return du, dattn, gout, dgamma, dbeta, dwo, None, None


def stu_output(u: torch.Tensor, attn: torch.Tensor, x: torch.Tensor, norm_weight: torch.Tensor, norm_bias: torch.Tensor,
               output_weight: torch.Tensor, num_heads: int, group_norm: bool, dropout_ratio: float, training: bool, eps: float = 1e-6,
               seed: Optional[torch.Tensor] = None, double_backward: bool = False) -> torch.Tensor:
    """x + dropout([silu(u), attn, silu(u) norm(attn)]) @ output_weight: u the RAW [L, H Dv] slice of the uvqk matrix, attn [L, H Dv],
    x [L, E].  `seed`: a one-element int64 tensor on the device, taken as given (tests); by default one is drawn on the device per
    forward (nothing is read back: the op captures into a hipGraph, and a replay draws a new mask)."""
    if FUSED_STU_OUTPUT and not double_backward and (x.is_cuda or _lib.emulated()) and x.dtype == torch.float32 and u.dtype == torch.float32 and \
            attn.dtype == torch.float32 and stu_output_ok(u, attn, x, norm_weight, norm_bias, output_weight, num_heads, group_norm, dropout_ratio):
        drop = bool(training) and dropout_ratio > 0.0
        if drop and seed is None:
            seed = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=x.device)
        return _StuOutputFn.apply(u, attn, x, norm_weight, norm_bias, output_weight, seed if drop else None,
                                  (int(num_heads), bool(group_norm), float(dropout_ratio), bool(training), float(eps)))
    return stu_output_literal(u, attn, x, norm_weight, norm_bias, output_weight, num_heads, group_norm, dropout_ratio, training, eps)


class STULayer(nn.Module):
    """One STU layer (constructor arguments and parameter names of the reference's STULayer): LayerNorm(eps 1e-6) -> addmm with
    `_uvqk_weight` -> split u, v, q, k -> `hstu_mha` on the slices where the product left them (no copy) -> `stu_output` on the raw
    u slice: silu(u) * norm(attn) (layer or group norm) -> [u, attn, y] -> dropout -> addmm(x, ., `_output_weight`).  `recompute_*` and
    `sort_by_length` are accepted and change no result."""

    def __init__(self, embedding_dim: int, num_heads: int, hidden_dim: int, attention_dim: int, output_dropout_ratio: float = 0.3,
                 causal: bool = True, target_aware: bool = True, max_attn_len: Optional[int] = None, attn_alpha: Optional[float] = None,
                 use_group_norm: bool = False, recompute_normed_x: bool = True, recompute_uvqk: bool = True, recompute_y: bool = True,
                 sort_by_length: bool = True, contextual_seq_len: int = 0, sla_k1: int = 0, sla_k2: int = 0, scaling_seqlen: int = -1,
                 is_inference: bool = False) -> None:
        super().__init__()
        if sla_k1 > 0 or sla_k2 > 0:
            raise NotImplementedError("STULayer: sla_k1 / sla_k2 (SLA masks) are not built")
        if not causal:
            raise NotImplementedError("STULayer: causal=False is not built")
        self.reset_kv_cache()
        self._num_heads, self._embedding_dim, self._hidden_dim, self._attention_dim = num_heads, embedding_dim, hidden_dim, attention_dim
        self._output_dropout_ratio, self._target_aware = output_dropout_ratio, target_aware
        self._max_attn_len = max_attn_len or 0
        self._attn_alpha = attn_alpha or 1.0 / (attention_dim ** 0.5)
        self._use_group_norm, self._contextual_seq_len, self._scaling_seqlen = use_group_norm, contextual_seq_len, scaling_seqlen
        width = (hidden_dim * 2 + attention_dim * 2) * num_heads
        self._uvqk_weight = nn.Parameter(torch.empty(embedding_dim, width))
        nn.init.xavier_uniform_(self._uvqk_weight)
        self._uvqk_beta = nn.Parameter(torch.zeros(width))
        self._input_norm_weight = nn.Parameter(torch.ones(embedding_dim))
        self._input_norm_bias = nn.Parameter(torch.zeros(embedding_dim))
        self._output_weight = nn.Parameter(torch.empty(hidden_dim * num_heads * 3, embedding_dim))
        nn.init.xavier_uniform_(self._output_weight)
        norm_shape = num_heads if use_group_norm else hidden_dim * num_heads
        self._output_norm_weight = nn.Parameter(torch.ones(norm_shape))
        self._output_norm_bias = nn.Parameter(torch.zeros(norm_shape))

    def forward(self, x: torch.Tensor, x_offsets: torch.Tensor, max_seq_len: int, num_targets: Optional[torch.Tensor] = None,
                max_kv_caching_len: int = 0, kv_caching_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """With `kv_caching_lengths` [B] (prefill) the first kv_caching_lengths[b] rows of k and v of every sample are kept as the
        layer's cache (the reference's _update_kv_cache).  max_kv_caching_len == 0 reads their maximum back once, as the reference
        does: a prefill captures into a hipGraph only with max_kv_caching_len given."""
        H, Dv, Da = self._num_heads, self._hidden_dim, self._attention_dim
        u, v, q, k = self._uvqk(x)
        self.update_kv_cache(max_seq_len, x_offsets, k, v, max_kv_caching_len, kv_caching_lengths)
        L = x.shape[0]
        attn = hstu_mha(max_seq_len, self._attn_alpha, q.view(L, H, Da), k.view(L, H, Da), v.view(L, H, Dv), x_offsets,
                        num_targets=num_targets if self._target_aware else None, max_attn_len=self._max_attn_len,
                        contextual_seq_len=self._contextual_seq_len, scaling_seqlen=self._scaling_seqlen).reshape(L, H * Dv)
        return stu_output(u, attn, x, self._output_norm_weight, self._output_norm_bias, self._output_weight, H, self._use_group_norm,
                          self._output_dropout_ratio, self.training)

    def _uvqk(self, x: torch.Tensor):
        """input norm and the uvqk product -> the u, v, q, k column slices [rows, H D] where the product left them"""
        H, Dv, Da = self._num_heads, self._hidden_dim, self._attention_dim
        normed = F.layer_norm(x, (self._embedding_dim,), self._input_norm_weight, self._input_norm_bias, 1e-6)
        uvqk = torch.addmm(self._uvqk_beta, normed, self._uvqk_weight)
        return torch.split(uvqk, [Dv * H, Dv * H, Da * H, Da * H], dim=1)

    def reset_kv_cache(self) -> None:
        self.k_cache: Optional[torch.Tensor] = None  # [rows, H Da]; the rows behind kv_caching_offsets[B] are spare
        self.v_cache: Optional[torch.Tensor] = None  # [rows, H Dv]
        self.kv_caching_offsets: Optional[torch.Tensor] = None
        self.max_kv_caching_len = 0

    def update_kv_cache(self, max_seq_len: int, seq_offsets: torch.Tensor, k: torch.Tensor, v: torch.Tensor, max_kv_caching_len: int,
                        kv_caching_lengths: Optional[torch.Tensor]) -> None:
        """The reference's _update_kv_cache: with kv_caching_lengths [B], the first kv_caching_lengths[b] rows of k, v [L, H D] of
        every sample, packed sample after sample, replace the cache; without, the cache stays.  The packed rows are written into
        buffers of L + 1 rows (the count of kept rows is not read back; the last row takes the rows that are not kept)."""
        if kv_caching_lengths is None:
            return
        L, B, dev = k.shape[0], seq_offsets.numel() - 1, k.device
        offsets = torch.cat([kv_caching_lengths.new_zeros(1), kv_caching_lengths.cumsum(0)]).to(torch.int64)
        pos = torch.arange(L, device=dev)
        b = torch.bucketize(pos, seq_offsets[1:], right=True).clamp(max=max(B - 1, 0))
        pos = pos - seq_offsets[b]
        dst = torch.where((pos >= 0) & (pos < kv_caching_lengths[b]), offsets[b] + pos, torch.full_like(pos, L)) if B > 0 else torch.full_like(pos, L)
        self.k_cache = k.new_zeros(L + 1, k.shape[1]).index_copy_(0, dst, k.detach())
        self.v_cache = v.new_zeros(L + 1, v.shape[1]).index_copy_(0, dst, v.detach())
        self.kv_caching_offsets = offsets
        self.max_kv_caching_len = int(max_kv_caching_len) if max_kv_caching_len > 0 else (int(kv_caching_lengths.max().item()) if B > 0 else 0)

    def construct_full_kv(self, delta_k: torch.Tensor, delta_v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int, torch.Tensor]:
        """The reference's _construct_full_kv out of torch ops: the cached rows of every sample followed by its rows of delta_k, delta_v
        [B delta, H D] -> (full_k, full_v, max_kv_caching_len + delta, their offsets).  `cached_forward` needs it only for a re-split."""
        delta = delta_k.shape[0] // (self.kv_caching_offsets.numel() - 1)
        full_k, offsets = concat_cache_delta(self.k_cache, delta_k, self.kv_caching_offsets, delta)
        full_v, _ = concat_cache_delta(self.v_cache, delta_v, self.kv_caching_offsets, delta)
        return full_k, full_v, self.max_kv_caching_len + delta, offsets

    def cached_forward(self, delta_x: torch.Tensor, num_targets: Optional[torch.Tensor], max_kv_caching_len: int = 0,
                       kv_caching_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The layer on delta = delta_x.shape[0] // B new rows a sample behind the cached ones (the reference's cached_forward): norm
        and uvqk on the delta rows, `delta_hstu_mha` in its two-segment form on the cache and the delta slices of uvqk where they lie
        (full_k / full_v are not built), `stu_output`.  With `kv_caching_lengths` (a re-split of cache + delta into a new cache) the
        full rows are built with torch ops as the reference does, and the attention takes them in the one-segment form."""
        if self.kv_caching_offsets is None:
            raise RuntimeError("STULayer.cached_forward: no kv cache (run forward with kv_caching_lengths first)")
        H, Dv, Da, Ld = self._num_heads, self._hidden_dim, self._attention_dim, delta_x.shape[0]
        u, v, q, k = self._uvqk(delta_x)
        B = self.kv_caching_offsets.numel() - 1
        kw = dict(num_targets=num_targets if self._target_aware else None, max_attn_len=self._max_attn_len,
                  contextual_seq_len=self._contextual_seq_len, scaling_seqlen=self._scaling_seqlen)
        if kv_caching_lengths is None:
            attn = delta_hstu_mha(self.max_kv_caching_len + Ld // max(B, 1), self._attn_alpha, q.view(Ld, H, Da), self.k_cache.view(-1, H, Da),
                                  self.v_cache.view(-1, H, Dv), self.kv_caching_offsets, delta_k=k.view(Ld, H, Da), delta_v=v.view(Ld, H, Dv), **kw)
        else:
            full_k, full_v, max_seq_len, offsets = self.construct_full_kv(k, v)
            self.update_kv_cache(max_seq_len, offsets, full_k, full_v, max_kv_caching_len, kv_caching_lengths)
            attn = delta_hstu_mha(max_seq_len, self._attn_alpha, q.view(Ld, H, Da), full_k.view(-1, H, Da), full_v.view(-1, H, Dv), offsets, **kw)
        return stu_output(u, attn.reshape(Ld, H * Dv), delta_x, self._output_norm_weight, self._output_norm_bias, self._output_weight, H,
                          self._use_group_norm, self._output_dropout_ratio, self.training)


class STUStack(nn.Module):
    """The layers in order (the reference's STUStack without mid-stack truncation)"""

    def __init__(self, stu_list: Sequence[nn.Module], truncate_split_layer: int = 0, truncate_tail_len: int = 0, is_inference: bool = False) -> None:
        super().__init__()
        if truncate_split_layer > 0 or truncate_tail_len > 0:
            raise NotImplementedError("STUStack: truncate_split_layer / truncate_tail_len (mid-stack truncation) are not built")
        self._stu_layers = nn.ModuleList(stu_list)

    def forward(self, x: torch.Tensor, x_offsets: torch.Tensor, max_seq_len: int, num_targets: Optional[torch.Tensor] = None,
                max_kv_caching_len: int = 0, kv_caching_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        for layer in self._stu_layers:
            x = layer(x, x_offsets, max_seq_len, num_targets, max_kv_caching_len, kv_caching_lengths)
        return x

    def cached_forward(self, delta_x: torch.Tensor, num_targets: Optional[torch.Tensor], max_kv_caching_len: int = 0,
                       kv_caching_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the layers' `cached_forward` in order, each against its own cache"""
        for layer in self._stu_layers:
            delta_x = layer.cached_forward(delta_x, num_targets, max_kv_caching_len, kv_caching_lengths)
        return delta_x


# ---- the positional and timestamp encoder in front of the stack ---------------------------------------------------------------
_TIME_FNS = ("sqrt", "log")


def _position_literal(alpha, max_seq_len, c, pos_w, ts_w, seq_offsets, seq_embeddings, timestamps, num_targets, interleave_targets,
                      time_bucket_fn, time_bucket_increments, query_time):
    """Both reference ops out of plain torch ops (ts_w None: the positional one): the index matrices [B, N] of
    pt_position.py, two gathers [B, N, E], and their sum added to alpha x on the rows a sample keeps.  Padded as `hstu_mha_literal`
    pads; rows at or behind max_seq_len and rows no sample owns get alpha x alone."""
    L, B, N, dev = seq_embeddings.shape[0], seq_offsets.numel() - 1, int(max_seq_len), seq_embeddings.device
    out = seq_embeddings * alpha
    if B <= 0 or L == 0:
        return out
    n = seq_offsets[1:] - seq_offsets[:-1]
    col = torch.arange(N, device=dev).view(1, N).expand(B, N)
    keep = col < n.view(-1, 1)
    rows = (seq_offsets[:-1].view(-1, 1) + col) % (L + 1)
    high = n if num_targets is None else n - num_targets * (2 if interleave_targets else 1)
    P = pos_w.shape[0]
    if ts_w is None:
        high = torch.clamp(high, max=P - 1).view(-1, 1)
        dense = pos_w[torch.minimum(col, high).clamp(min=0)]
    else:
        high = high.view(-1, 1)
        idx = torch.clamp(high - torch.minimum(col, high) + c, max=P - 1)
        idx = torch.where(col < c, col, idx)
        T = ts_w.shape[0] - 1
        tm = torch.cat([timestamps, timestamps.new_zeros(1)])[rows]
        qt = timestamps[(seq_offsets[1:] - 1).clamp(0, L - 1)] if query_time is None else query_time.to(timestamps.dtype)
        u = (qt.view(-1, 1) - tm).clamp(min=1e-6) / time_bucket_increments
        u = torch.log(u) if time_bucket_fn == "log" else torch.sqrt(u)
        bucket = ((u / T).clamp(min=0, max=1) * T).int()
        dense = ts_w[bucket] + pos_w[idx]
    return out.index_put((rows[keep],), dense[keep].to(out.dtype), accumulate=True)


def add_positional_embeddings_literal(alpha: float, max_seq_len: int, position_embeddings_weight: torch.Tensor, seq_offsets: torch.Tensor,
                                      seq_lengths: Optional[torch.Tensor], seq_embeddings: torch.Tensor, num_targets: Optional[torch.Tensor],
                                      interleave_targets: bool) -> torch.Tensor:
    """pytorch_add_position_embeddings out of plain torch ops (no fbgemm)"""
    return _position_literal(alpha, max_seq_len, 0, position_embeddings_weight, None, seq_offsets, seq_embeddings, None, num_targets,
                             interleave_targets, "sqrt", 1.0, None)


def add_timestamp_positional_embeddings_literal(alpha: float, max_seq_len: int, max_contextual_seq_len: int, position_embeddings_weight: torch.Tensor,
                                                timestamp_embeddings_weight: torch.Tensor, seq_offsets: torch.Tensor,
                                                seq_lengths: Optional[torch.Tensor], seq_embeddings: torch.Tensor, timestamps: torch.Tensor,
                                                num_targets: Optional[torch.Tensor], interleave_targets: bool, time_bucket_fn: str = "sqrt",
                                                time_bucket_increments: float = 60.0, query_time: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pytorch_add_timestamp_positional_embeddings behind `seq_embeddings * alpha`, out of plain torch ops (no fbgemm)"""
    return _position_literal(alpha, max_seq_len, int(max_contextual_seq_len), position_embeddings_weight, timestamp_embeddings_weight, seq_offsets,
                             seq_embeddings, timestamps, num_targets, interleave_targets, time_bucket_fn, time_bucket_increments, query_time)


def hstu_position_limit(E: int, P: int, max_seq_len: int, T: Optional[int] = None, contextual_seq_len: int = 0,
                        dtype: torch.dtype = torch.float32) -> Optional[str]:
    """None when tzr_hstu_pos_* has a kernel for the shape (T None: the positional op), else the limit of csrc/hstu_position.hip it
    misses (include/tzrec_hip.h)"""
    if dtype not in (torch.float32, torch.bfloat16):
        return f"dtype {dtype} must be float32 or bfloat16"
    step, D = 8 if dtype == torch.bfloat16 else 4, _lib.HSTU_POS_MAX_DIM
    if E % step or not step <= E <= D:
        return f"embedding_dim {E} must be a multiple of {step} in [{step}, {D}]"
    if P < 1:
        return f"position buckets {P} must be at least 1"
    if not 1 <= max_seq_len <= _lib.HSTU_MAX_SEQ_LEN:
        return f"max_seq_len {max_seq_len} must be in [1, {_lib.HSTU_MAX_SEQ_LEN}]"
    if T is not None and not 1 <= T <= _lib.HSTU_POS_MAX_BUCKETS:
        return f"time buckets {T} must be in [1, {_lib.HSTU_POS_MAX_BUCKETS}]"
    if T is not None and not 0 <= contextual_seq_len <= P:
        return f"max_contextual_seq_len {contextual_seq_len} must be in [0, {P}] (the position buckets)"
    return None


def _rows16_ok(t: torch.Tensor) -> bool:
    """[L, E] fp32 or bf16 whose rows the 16-byte accesses take: unit column stride, rows a multiple of 16 bytes and a whole width
    apart, 16-byte aligned data (a column slice of a wider matrix passes)"""
    step = 8 if t.dtype == torch.bfloat16 else 4
    stride = _lib.scalar_row_stride(t)
    return t.stride(1) == 1 and stride % step == 0 and stride >= t.shape[1] and t.data_ptr() % 16 == 0


def _int64_ok(t: Optional[torch.Tensor], shape: tuple, dev: torch.device) -> bool:
    return t is None or (t.shape == shape and t.dtype == torch.int64 and t.is_contiguous() and t.device == dev)


def hstu_position_ok(max_seq_len: int, position_embeddings_weight: torch.Tensor, seq_offsets: torch.Tensor, seq_embeddings: torch.Tensor,
                     num_targets: Optional[torch.Tensor] = None, timestamp_embeddings_weight: Optional[torch.Tensor] = None,
                     timestamps: Optional[torch.Tensor] = None, query_time: Optional[torch.Tensor] = None, max_contextual_seq_len: int = 0,
                     time_bucket_fn: str = "sqrt", time_bucket_increments: float = 60.0) -> bool:
    """what tzr_hstu_pos_* takes: seq_embeddings [L, E] and the tables [P, E], [T + 1, E] (contiguous) of ONE dtype, fp32 or bf16,
    the rows as `_rows16_ok` takes them; offsets [B + 1], num_targets [B], timestamps [L], query_time [B] int64 and contiguous; a
    shape inside `hstu_position_limit`; everything on the device of the loaded library"""
    x, pw, tw = seq_embeddings, position_embeddings_weight, timestamp_embeddings_weight
    if x.dim() != 2 or pw.dim() != 2 or pw.shape[1] != x.shape[1] or seq_offsets.dim() != 1 or seq_offsets.numel() < 1 or x.shape[0] >= 2 ** 31:
        return False
    dev, (L, E), B = x.device, x.shape, seq_offsets.numel() - 1
    if not _lib.takes(x) or pw.dtype != x.dtype or pw.device != dev or not pw.is_contiguous() or pw.data_ptr() % 16:
        return False
    if tw is not None:
        if tw.dim() != 2 or tw.shape[1] != E or tw.shape[0] < 2 or tw.dtype != x.dtype or tw.device != dev or not tw.is_contiguous() or tw.data_ptr() % 16:
            return False
        if timestamps is None or not _int64_ok(timestamps, (L,), dev) or not _int64_ok(query_time, (B,), dev):
            return False
        if time_bucket_fn not in _TIME_FNS or not time_bucket_increments > 0:
            return False
    if hstu_position_limit(E, pw.shape[0], max_seq_len, None if tw is None else tw.shape[0] - 1, max_contextual_seq_len, x.dtype) is not None:
        return False
    if not _int64_ok(seq_offsets, (B + 1,), dev) or not _int64_ok(num_targets, (B,), dev):
        return False
    return L == 0 or _rows16_ok(x)


def _pos_fill(m, cfg, dtype, E, P, T, seq_offsets, num_targets, bucket):
    max_seq_len, alpha, c, interleave, fn, incr = cfg
    m.B, m.E, m.P, m.T, m.max_seq_len, m.contextual_seq_len = seq_offsets.numel() - 1, E, P, T or 0, max_seq_len, c
    m.use_time, m.interleave_targets, m.time_fn, m.bf16 = int(T is not None), int(interleave), fn, int(dtype == torch.bfloat16)
    m.alpha, m.time_bucket_increments = alpha, incr
    m.offsets, m.num_targets, m.bucket = _lib.ptr(seq_offsets), _lib.opt_ptr(num_targets), _lib.opt_ptr(bucket)


def hstu_pos_fwd(x, pos_w, ts_w, seq_offsets, num_targets, timestamps, query_time, cfg) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """tzr_hstu_pos_fwd on operands `hstu_position_ok` took -> out [L, E] (the kernel writes every row) and, with a timestamp
    table, the rows' buckets int32 [L]"""
    (L, E), dev = x.shape, x.device
    out = torch.empty(L, E, dtype=x.dtype, device=dev)
    bucket = None if ts_w is None else torch.empty(L, dtype=torch.int32, device=dev)
    if L > 0:
        m = _lib.TzrHstuPos()
        _pos_fill(m, cfg, x.dtype, E, pos_w.shape[0], None if ts_w is None else ts_w.shape[0] - 1, seq_offsets, num_targets, bucket)
        m.L, m.x, m.x_stride, m.out, m.out_stride = L, _lib.ptr(x), _lib.scalar_row_stride(x), _lib.ptr(out), E
        m.pos, m.ts, m.timestamps, m.query_time = _lib.ptr(pos_w), _lib.opt_ptr(ts_w), _lib.opt_ptr(timestamps), _lib.opt_ptr(query_time)
        _lib.launch("tzr_hstu_pos_fwd", m, dev)
    return out, bucket


def hstu_pos_bwd(gout, dtype, P, T, seq_offsets, num_targets, bucket, cfg):
    """tzr_hstu_pos_bwd -> dx [L, E], dpos [P, E], dts [T + 1, E] or None; every element written by the kernels"""
    (L, E), dev = gout.shape, gout.device
    g = gout.to(dtype)
    if L > 0 and not _rows16_ok(g):
        g = g.clone(memory_format=torch.contiguous_format)
    dx, dpos = torch.empty(L, E, dtype=dtype, device=dev), torch.empty(P, E, dtype=dtype, device=dev)
    dts = None if T is None else torch.empty(T + 1, E, dtype=dtype, device=dev)
    m = _lib.TzrHstuPos()
    _pos_fill(m, cfg, dtype, E, P, T, seq_offsets, num_targets, bucket if L > 0 else None)
    m.L, m.dpos, m.dts = L, _lib.ptr(dpos), _lib.opt_ptr(dts)
    if L > 0:
        m.grad_out, m.grad_out_stride, m.dx, m.dx_stride = _lib.ptr(g), _lib.scalar_row_stride(g), _lib.ptr(dx), E
    _lib.launch_ws("tzr_hstu_pos_bwd", m, dev, "tzr_hstu_pos_bwd")
    return dx, dpos, dts


class _HstuPositionFn(torch.autograd.Function):
    """Saved for the backward: the offsets, num_targets and the int32 buckets -- no row of x, no timestamp.  Capturable: every
    buffer is torch's, the workspace included; nothing is read back.  Differentiable once (a double backward takes the literal form)."""

    calls = 0  # forwards that took the kernel (tests)

    @staticmethod
    def forward(ctx, x, pos_w, ts_w, seq_offsets, num_targets, timestamps, query_time, cfg):
        _HstuPositionFn.calls += 1
        out, bucket = hstu_pos_fwd(x.detach(), pos_w.detach(), None if ts_w is None else ts_w.detach(), seq_offsets, num_targets, timestamps, query_time, cfg)
        ctx.save_for_backward(seq_offsets, num_targets, bucket)
        ctx.cfg, ctx.shape = cfg, (x.dtype, pos_w.shape[0], None if ts_w is None else ts_w.shape[0] - 1)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        dx, dpos, dts = hstu_pos_bwd(gout, *ctx.shape, *ctx.saved_tensors, ctx.cfg)
        return dx, dpos, dts, None, None, None, None, None


def _position(alpha, max_seq_len, c, pos_w, ts_w, seq_offsets, x, timestamps, num_targets, interleave_targets, time_bucket_fn,
              time_bucket_increments, query_time, double_backward):
    max_seq_len, c = int(max_seq_len), int(c)
    if FUSED_HSTU_POSITION and not double_backward and (x.is_cuda or _lib.emulated()) and \
            hstu_position_ok(max_seq_len, pos_w, seq_offsets, x, num_targets, ts_w, timestamps, query_time, c, time_bucket_fn, time_bucket_increments):
        cfg = (max_seq_len, float(alpha), c, bool(interleave_targets), _TIME_FNS.index(time_bucket_fn), float(time_bucket_increments))
        return _HstuPositionFn.apply(x, pos_w, ts_w, seq_offsets, num_targets, timestamps, query_time, cfg)
    return _position_literal(alpha, max_seq_len, c, pos_w, ts_w, seq_offsets, x, timestamps, num_targets, interleave_targets, time_bucket_fn,
                             time_bucket_increments, query_time)


def add_positional_embeddings(alpha: float, max_seq_len: int, position_embeddings_weight: torch.Tensor, seq_offsets: torch.Tensor,
                              seq_lengths: Optional[torch.Tensor], seq_embeddings: torch.Tensor, num_targets: Optional[torch.Tensor],
                              interleave_targets: bool, double_backward: bool = False) -> torch.Tensor:
    """The reference's add_positional_embeddings: row i of a sample with n rows gets alpha x + pos[min(i, high)], high =
    min(n - num_targets (twice under interleave_targets), P - 1); [L, E] -> [L, E].  `seq_lengths` is accepted; the offsets are
    what is read.  Rows at or behind max_seq_len of a sample get alpha x alone."""
    return _position(alpha, max_seq_len, 0, position_embeddings_weight, None, seq_offsets, seq_embeddings, None, num_targets, interleave_targets,
                     "sqrt", 1.0, None, double_backward)


def add_timestamp_positional_embeddings(alpha: float, max_seq_len: int, max_contextual_seq_len: int, position_embeddings_weight: torch.Tensor,
                                        timestamp_embeddings_weight: torch.Tensor, seq_offsets: torch.Tensor, seq_lengths: Optional[torch.Tensor],
                                        seq_embeddings: torch.Tensor, timestamps: torch.Tensor, num_targets: Optional[torch.Tensor],
                                        interleave_targets: bool, time_bucket_fn: str = "sqrt", time_bucket_increments: float = 60.0,
                                        query_time: Optional[torch.Tensor] = None, double_backward: bool = False) -> torch.Tensor:
    """The reference's add_timestamp_positional_embeddings: alpha x + pos[idx] + ts[bucket] by the rule of include/tzrec_hip.h (the
    position counted back from the first target, the contextual prefix on its own rows; the bucket from the gap to `query_time`,
    by default the timestamp of the sample's last row).  On csrc/hstu_position.hip when FUSED_HSTU_POSITION is on and
    `hstu_position_ok` takes the operands, else the literal form."""
    if time_bucket_fn not in _TIME_FNS:
        raise ValueError(f"time_bucket_fn {time_bucket_fn!r} must be one of {_TIME_FNS}")
    return _position(alpha, max_seq_len, max_contextual_seq_len, position_embeddings_weight, timestamp_embeddings_weight, seq_offsets, seq_embeddings,
                     timestamps, num_targets, interleave_targets, time_bucket_fn, time_bucket_increments, query_time, double_backward)


class HSTUPositionalEncoder(nn.Module):
    """The reference's HSTUPositionalEncoder (constructor arguments, parameter names and initialisation): `_position_embeddings_weight`
    [num_position_buckets, E] and, with use_time_encoding, `_timestamp_embeddings_weight` [num_time_buckets + 1, E], added to
    sqrt(E) x by `add_timestamp_positional_embeddings` / `add_positional_embeddings`."""

    def __init__(self, embedding_dim: int, num_position_buckets: int, num_time_buckets: int = 0, use_time_encoding: bool = False,
                 contextual_seq_len: int = 0, time_bucket_fn: str = "sqrt", time_bucket_increments: float = 60.0, is_inference: bool = True) -> None:
        super().__init__()
        self._use_time_encoding, self._contextual_seq_len, self._embedding_dim = use_time_encoding, contextual_seq_len, embedding_dim
        bound = (1.0 / num_position_buckets) ** 0.5
        self._position_embeddings_weight = nn.Parameter(torch.empty(num_position_buckets, embedding_dim).uniform_(-bound, bound))
        if use_time_encoding:
            bound = (1.0 / num_time_buckets) ** 0.5
            self._timestamp_embeddings_weight = nn.Parameter(torch.empty(num_time_buckets + 1, embedding_dim).uniform_(-bound, bound))
            self._time_bucket_fn, self._time_bucket_increments = time_bucket_fn, time_bucket_increments

    def forward(self, max_seq_len: int, seq_lengths: torch.Tensor, seq_offsets: torch.Tensor, seq_timestamps: torch.Tensor,
                seq_embeddings: torch.Tensor, num_targets: Optional[torch.Tensor], query_time: Optional[torch.Tensor] = None) -> torch.Tensor:
        alpha = self._embedding_dim ** 0.5
        if self._use_time_encoding:
            return add_timestamp_positional_embeddings(alpha, max_seq_len, self._contextual_seq_len, self._position_embeddings_weight,
                                                       self._timestamp_embeddings_weight, seq_offsets, seq_lengths, seq_embeddings, seq_timestamps,
                                                       num_targets, False, self._time_bucket_fn, self._time_bucket_increments, query_time)
        return add_positional_embeddings(alpha, max_seq_len, self._position_embeddings_weight, seq_offsets, seq_lengths, seq_embeddings, num_targets, False)
