"""HSTU's contextualized MLPs (tzrec/modules/gr/contextualize_mlps.py: SimpleContextualizedMLP, ParameterizedContextualizedMLP,
create_contextualized_mlp), the layers of the input preprocessor that turn content and action rows into STU rows, and the jagged
matmul under the parameterized one (tzrec/ops/jagged_tensors.py::jagged_dense_bmm_broadcast_add).

`jagged_dense_bmm_broadcast_add` is out[r] = jagged[r] @ dense[b(r)] + bias[b(r)]: a [K, N] matrix and a bias row per sample on a
jagged batch.  It runs csrc/jagged_bmm.hip (tzr_jagged_bmm_fwd / _bwd: one launch forward, two backward, on the fp32 MFMAs; d_dense
and d_bias are fixed-order sums over a sample's rows, no atomics, no workspace; nothing of size [B, max_seq_len, .] is in memory, the
work follows the rows) when FUSED_JAGGED_BMM is on and `jagged_bmm_ok` takes the operands; otherwise -- the switch off, bf16, fp16 or
mixed dtypes, a shape outside `jagged_bmm_limit`, a double backward -- `jagged_dense_bmm_broadcast_add_literal`, the reference's
padded form [B, max_seq_len, K] out of plain torch ops.  A sample keeps its first max_seq_len rows; the rows behind them, and rows
behind seq_offsets[B], get zero output and zero gradient and take no part in d dense or d bias: the rule of `hstu.hstu_mha`.

What stays torch ops in the two modules: every Linear, LayerNorm and SwishLayerNorm, and the dropout of the contextual embeddings."""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

# profiles/jagged_bmm, forward + backward at 38 866 rows of 16 samples, N = 512: K = 64 539.4 us fused (536.8 - 584.5) against 845.1 us
# literal (836.9 - 881.0), 92 against 408 MB; K = 256 930.4 us (925.7 - 1 440.8) against 1 177.7 us (1 168.4 - 1 226.6), 128 against 508 MB
FUSED_JAGGED_BMM = True


def jagged_dense_bmm_broadcast_add_literal(max_seq_len: int, seq_offsets: torch.Tensor, jagged: torch.Tensor, dense: torch.Tensor,
                                           bias: torch.Tensor) -> torch.Tensor:
    """The reference's padded form (pytorch_jagged_dense_bmm_broadcast_add) out of plain torch ops: upcasts to fp32, gathers the rows
    into [B, max_seq_len, K], one bmm over all B x max_seq_len positions, scatters back; [L, K] -> [L, N] in jagged's dtype."""
    (L, K), N, B = jagged.shape, int(max_seq_len), seq_offsets.numel() - 1
    n = torch.clamp(seq_offsets[1:] - seq_offsets[:-1], max=N)
    pos = torch.arange(N, device=jagged.device).view(1, N)
    keep = pos < n.view(-1, 1)
    # (a position a sample does not have reads a later row, wrapping over a spare zero row, and is zeroed by `keep`: no shared
    # padding row to take every padded position's gradient -- hstu.hstu_mha_literal)
    idx = (seq_offsets[:-1].view(-1, 1) + pos) % (L + 1)
    x = jagged.to(torch.float32)
    rows = torch.cat([x, x.new_zeros(1, K)])[idx]  # [B, N, K]
    padded = torch.where(keep.unsqueeze(2), rows, rows.new_zeros(()))
    res = torch.bmm(padded, dense.to(torch.float32)) + bias.unsqueeze(1)
    return res.new_zeros(L, dense.shape[2]).index_put((idx[keep],), res[keep]).to(jagged.dtype)


def jagged_bmm_limit(K: int, N: int, max_seq_len: int, B: int = 1, dtype: torch.dtype = torch.float32) -> Optional[str]:
    """None when tzr_jagged_bmm_* has a kernel for the shape, else the limit of csrc/jagged_bmm.hip it misses (include/tzrec_hip.h)"""
    D = _lib.JAGGED_BMM_MAX_DIM
    if dtype != torch.float32:
        return f"dtype {dtype} must be float32"
    for name, d in (("K", K), ("N", N)):
        if d % 4 or not 4 <= d <= D:
            return f"{name} {d} must be a multiple of 4 in [4, {D}]"
    if not 1 <= max_seq_len <= _lib.HSTU_MAX_SEQ_LEN:
        return f"max_seq_len {max_seq_len} must be in [1, {_lib.HSTU_MAX_SEQ_LEN}]"
    block, chunks = _lib.JAGGED_BMM_BLOCK, (max(K, N) + _lib.JAGGED_BMM_CHUNK - 1) // _lib.JAGGED_BMM_CHUNK
    if max((max_seq_len + block - 1) // block, 2 * chunks) * chunks * max(B, 1) >= 2 ** 31:
        return f"grid: ceil({max_seq_len} / {block}) x {chunks} x {B} workgroups must stay below 2^31"
    return None


def jagged_bmm_ok(max_seq_len: int, seq_offsets: torch.Tensor, jagged: torch.Tensor, dense: torch.Tensor, bias: torch.Tensor) -> bool:
    """what tzr_jagged_bmm_* takes: jagged [L, K] a `_lib.rows_ok` operand (a column slice of a wider matrix is), dense [B, K, N] and
    bias [B, N] fp32, contiguous and 16-byte aligned, offsets int64 [B + 1] contiguous, a shape inside `jagged_bmm_limit`, everything
    on the device of the loaded library"""
    if jagged.dim() != 2 or dense.dim() != 3 or bias.dim() != 2 or seq_offsets.dim() != 1 or seq_offsets.numel() < 1:
        return False
    dev, (L, K), (B, _, N) = jagged.device, jagged.shape, dense.shape
    if not _lib.takes(jagged) or L >= 2 ** 31 or jagged.dtype != torch.float32 or dense.shape[1] != K:
        return False
    if not _lib.packed_ok(dense, (B, K, N), dev, aligned=True) or not _lib.packed_ok(bias, (B, N), dev, aligned=True):
        return False
    if seq_offsets.shape != (B + 1,) or seq_offsets.dtype != torch.int64 or not seq_offsets.is_contiguous() or seq_offsets.device != dev:
        return False
    if jagged_bmm_limit(K, N, max_seq_len, B) is not None:
        return False
    return L == 0 or _lib.rows_ok(jagged)


def _fill(m, max_seq_len, seq_offsets, jagged, dense):
    m.L, m.B, m.K, m.N, m.max_seq_len = jagged.shape[0], dense.shape[0], dense.shape[1], dense.shape[2], max_seq_len
    m.jagged, m.jagged_stride = _lib.ptr(jagged), _lib.scalar_row_stride(jagged)
    m.dense, m.offsets = _lib.ptr(dense), _lib.ptr(seq_offsets)


def jagged_bmm_fwd(max_seq_len, seq_offsets, jagged, dense, bias) -> torch.Tensor:
    """tzr_jagged_bmm_fwd on operands `jagged_bmm_ok` took -> out [L, N] (torch.empty: the kernel writes every row); no sample or no
    row: zeros without a launch"""
    L, (B, _, N) = jagged.shape[0], dense.shape
    if B == 0 or L == 0:
        return jagged.new_zeros(L, N)
    out = torch.empty(L, N, dtype=jagged.dtype, device=jagged.device)
    m = _lib.TzrJaggedBmm()
    _fill(m, max_seq_len, seq_offsets, jagged, dense)
    m.bias, m.out, m.out_stride = _lib.ptr(bias), _lib.ptr(out), N
    _lib.launch("tzr_jagged_bmm_fwd", m, jagged.device)
    return out


def jagged_bmm_bwd(gout, max_seq_len, seq_offsets, jagged, dense) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """tzr_jagged_bmm_bwd -> d jagged [L, K], d dense [B, K, N], d bias [B, N]; every element written by the kernels"""
    (L, K), (B, _, N), dev = jagged.shape, dense.shape, jagged.device
    if B == 0 or L == 0:
        return jagged.new_zeros(L, K), dense.new_zeros(B, K, N), dense.new_zeros(B, N)
    g = gout.to(jagged.dtype)
    if not _lib.rows_ok(g):
        g = g.clone(memory_format=torch.contiguous_format)  # (.contiguous() keeps the odd strides of a one-row gradient: _lib.rows16)
    dj, dd, db = (torch.empty(s, dtype=jagged.dtype, device=dev) for s in ((L, K), (B, K, N), (B, N)))
    m = _lib.TzrJaggedBmm()
    _fill(m, max_seq_len, seq_offsets, jagged, dense)
    m.grad_out, m.grad_out_stride, m.d_jagged, m.d_jagged_stride = _lib.ptr(g), _lib.scalar_row_stride(g), _lib.ptr(dj), K
    m.d_dense, m.d_bias = _lib.ptr(dd), _lib.ptr(db)
    _lib.launch("tzr_jagged_bmm_bwd", m, dev)
    return dj, dd, db


class _JaggedBmmFn(torch.autograd.Function):
    """Saved for the backward: the inputs alone.  Capturable: every buffer is torch's, nothing is read back.  Differentiable once
    (`jagged_dense_bmm_broadcast_add(.., double_backward=True)` takes the literal form)."""

    calls = 0  # forwards that took the kernel (tests)

    @staticmethod
    def forward(ctx, jagged, dense, bias, seq_offsets, max_seq_len):
        _JaggedBmmFn.calls += 1
        ctx.save_for_backward(jagged, dense, seq_offsets)
        ctx.max_seq_len = max_seq_len
        return jagged_bmm_fwd(max_seq_len, seq_offsets, jagged.detach(), dense.detach(), bias.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        jagged, dense, seq_offsets = ctx.saved_tensors
        dj, dd, db = jagged_bmm_bwd(gout, ctx.max_seq_len, seq_offsets, jagged, dense)
        return dj, dd, db, None, None


def jagged_dense_bmm_broadcast_add(max_seq_len: int, seq_offsets: torch.Tensor, jagged: torch.Tensor, dense: torch.Tensor, bias: torch.Tensor,
                                   double_backward: bool = False) -> torch.Tensor:
    """The reference's jagged_dense_bmm_broadcast_add: jagged [L, K] by seq_offsets [B + 1], dense [B, K, N], bias [B, N] -> [L, N] in
    jagged's dtype, out[r] = jagged[r] @ dense[b] + bias[b] for the first max_seq_len rows of sample b, zeros for the others."""
    max_seq_len = int(max_seq_len)
    if FUSED_JAGGED_BMM and not double_backward and (jagged.is_cuda or _lib.emulated()) and \
            jagged.dtype == dense.dtype == bias.dtype == torch.float32 and jagged_bmm_ok(max_seq_len, seq_offsets, jagged, dense, bias):
        return _JaggedBmmFn.apply(jagged, dense, bias, seq_offsets, max_seq_len)
    return jagged_dense_bmm_broadcast_add_literal(max_seq_len, seq_offsets, jagged, dense, bias)


def _init_linear_xavier_weights_zero_bias(m: nn.Module) -> None:
    if isinstance(m, nn.Linear):
        nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            m.bias.data.fill_(0.0)


class SwishLayerNorm(nn.Module):
    """The reference's SwishLayerNorm (tzrec/modules/norm.py): x * sigmoid(layer_norm(x)), parameters `weight` and `bias` [dim]"""

    def __init__(self, dim: int, eps: float = 1e-5, is_inference: bool = False) -> None:
        super().__init__()
        self._normalized_shape, self._eps = [dim], eps
        self.weight, self.bias = nn.Parameter(torch.ones(dim)), nn.Parameter(torch.zeros(dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x * torch.sigmoid(F.layer_norm(x, self._normalized_shape, self.weight, self.bias, self._eps))


class SimpleContextualizedMLP(nn.Module):
    """The reference's SimpleContextualizedMLP (constructor arguments, parameter names `_mlp.0` .. `_mlp.3`, initialisation):
    Linear, SwishLayerNorm, Linear, LayerNorm on the rows; offsets and contextual embeddings are accepted and not read."""

    def __init__(self, sequential_input_dim: int, sequential_output_dim: int, hidden_dim: int, is_inference: bool = False, **kwargs: Any) -> None:
        super().__init__()
        self._mlp = nn.Sequential(nn.Linear(sequential_input_dim, hidden_dim), SwishLayerNorm(hidden_dim, is_inference=is_inference),
                                  nn.Linear(hidden_dim, sequential_output_dim), nn.LayerNorm(sequential_output_dim, eps=1e-5)
                                  ).apply(_init_linear_xavier_weights_zero_bias)

    def forward(self, seq_embeddings: torch.Tensor, seq_offsets: torch.Tensor, max_seq_len: int,
                contextual_embeddings: Optional[torch.Tensor]) -> torch.Tensor:
        return self._mlp(seq_embeddings)


class ParameterizedContextualizedMLP(nn.Module):
    """The reference's ParameterizedContextualizedMLP (constructor arguments, parameter names, initialisation): the contextual
    embeddings [B, contextual_embedding_dim] make, per sample, a layer-normed [K, N] matrix and a bias row [N], applied to the
    sample's rows by `jagged_dense_bmm_broadcast_add`; [L, K] -> [L, N]."""

    def __init__(self, contextual_embedding_dim: int, sequential_input_dim: int, sequential_output_dim: int, hidden_dim: int,
                 contextual_dropout_ratio: float = 0.3, is_inference: bool = False, **kwargs: Any) -> None:
        super().__init__()
        self._sequential_input_dim, self._sequential_output_dim = sequential_input_dim, sequential_output_dim
        self._contextual_dropout_ratio = contextual_dropout_ratio
        self._dense_features_compress = nn.Linear(contextual_embedding_dim, hidden_dim).apply(_init_linear_xavier_weights_zero_bias)
        self._attn_raw_weights = nn.Sequential(nn.Linear(hidden_dim, sequential_input_dim * sequential_output_dim)
                                               ).apply(_init_linear_xavier_weights_zero_bias)
        self._attn_weights_norm = nn.LayerNorm([sequential_input_dim, sequential_output_dim])
        self._res_weights = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), SwishLayerNorm(hidden_dim),
                                          nn.Linear(hidden_dim, sequential_output_dim)).apply(_init_linear_xavier_weights_zero_bias)

    def forward(self, seq_embeddings: torch.Tensor, seq_offsets: torch.Tensor, max_seq_len: int,
                contextual_embeddings: Optional[torch.Tensor]) -> torch.Tensor:
        assert contextual_embeddings is not None
        contextual_embeddings = F.dropout(contextual_embeddings, p=self._contextual_dropout_ratio, training=self.training)
        shared_input = self._dense_features_compress(contextual_embeddings)
        attn_weights = self._attn_weights_norm(
            self._attn_raw_weights(shared_input).reshape(-1, self._sequential_input_dim, self._sequential_output_dim))
        return jagged_dense_bmm_broadcast_add(max_seq_len, seq_offsets, seq_embeddings, attn_weights.to(seq_embeddings.dtype),
                                              self._res_weights(shared_input))


def create_contextualized_mlp(mlp_cfg: Dict[str, Any], **kwargs: Any) -> nn.Module:
    """The reference's create_contextualized_mlp in its dict form: {"simple_mlp": kwargs} or {"parameterized_mlp": kwargs}"""
    assert len(mlp_cfg) == 1, f"mlp_cfg should be {{mlp_type: mlp_kwargs}}, but got {mlp_cfg}"
    (mlp_type, config), = mlp_cfg.items()
    config = dict(config, **kwargs)
    if mlp_type == "simple_mlp":
        return SimpleContextualizedMLP(**config)
    if mlp_type == "parameterized_mlp":
        return ParameterizedContextualizedMLP(**config)
    raise RuntimeError(f"Unknown contextualized mlp type: {mlp_type}")
