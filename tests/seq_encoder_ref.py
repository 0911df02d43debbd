"""Padded pure-torch restatement of the two cheap sequence encoders (simple attention, sum / mean pooling) for the tests of
csrc/jagged_encoders.hip: the reference's formulas on a zero-padded [B, L, D] tensor, written without any code of the package
under test.  `rows` [N, D] jagged rows, `lengths` [B]; L = the padded length (positions behind it do not exist)."""
import torch


def pad_rows(rows: torch.Tensor, lengths, L: int) -> torch.Tensor:
    """jagged rows -> zero-padded [B, L, D] (differentiable: plain indexing)"""
    B, D = len(lengths), rows.shape[1]
    out = torch.zeros(B, L, D, dtype=rows.dtype) + 0 * rows.sum()  # (a batch without rows still depends on `rows`: zero gradient)
    start = 0
    for b, n in enumerate(int(x) for x in lengths):
        k = min(n, L)
        if k:
            out[b, :k] = rows[start:start + k]
        start += n
    return out


def simple_attention(query: torch.Tensor, rows: torch.Tensor, lengths, L: int, max_seq_length: int = 0) -> torch.Tensor:
    seq = pad_rows(rows, lengths, L)
    ln = torch.as_tensor(lengths, dtype=torch.int64)
    if max_seq_length > 0:
        ln, seq = torch.clamp_max(ln, max_seq_length), seq[:, :max_seq_length]
    mask = torch.arange(seq.shape[1]).unsqueeze(0) < ln.unsqueeze(1)
    s = torch.matmul(seq, query.unsqueeze(2)).squeeze(2)
    p = torch.softmax(torch.where(mask, s, torch.full_like(s, -(2.0 ** 31) + 1)), dim=-1)
    return torch.matmul(p.unsqueeze(1), seq).squeeze(1)


def pooling(rows: torch.Tensor, lengths, L: int, pooling_type: str = "mean", max_seq_length: int = 0) -> torch.Tensor:
    seq = pad_rows(rows, lengths, L)
    ln = torch.as_tensor(lengths, dtype=torch.int64)
    if max_seq_length > 0:
        ln, seq = torch.clamp_max(ln, max_seq_length), seq[:, :max_seq_length]
    out = seq.sum(dim=1)
    if pooling_type == "mean":
        out = out / torch.clamp(torch.clamp_max(ln, seq.shape[1]), min=1).unsqueeze(1)
    return out
