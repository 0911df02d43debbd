"""Restatement of the jagged matmul with per-sample weights for the tests: per sample the dense form
    out[rows of b] = jagged[rows of b] @ dense[b] + bias[b]        over the n = min(len, max_seq_len) rows a sample keeps,
zeros for every other row, in plain torch on the CPU in the dtype asked for; gradients by autograd against a fixed upstream
gradient.  In float64 it is the truth the kernels are held to; in float32 (or bfloat16) the yardstick (`gaps`).  Nothing here
touches the package under test."""
import torch

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

KINDS = ("out", "dj", "dd", "db")


def product(p, x, w, c):
    """x [L, K], w [B, K, N], c [B, N] of one dtype -> out [L, N]"""
    offsets, outs = p["offsets"].tolist(), []
    for b in range(len(offsets) - 1):
        s, ln = offsets[b], offsets[b + 1] - offsets[b]
        n = min(ln, p["max_seq_len"])
        outs += [x[s:s + n] @ w[b] + c[b], x.new_zeros(ln - n, w.shape[2])]
    outs.append(x.new_zeros(x.shape[0] - offsets[-1], w.shape[2]))  # spare rows behind offsets[B]
    return torch.cat(outs + [x[:0] @ x.new_zeros(x.shape[1], w.shape[2])])  # (an empty batch still hangs on x)


def literal(p, dtype=torch.float64):
    leaves = [p[k].detach().to(dtype).clone().requires_grad_(True) for k in ("jagged", "dense", "bias")]
    out = product(p, *leaves)
    grads = torch.autograd.grad((out * p["g"].to(dtype)).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    return {k: [t.detach().double()] for k, t in zip(KINDS, [out] + grads)}


def draw(lengths, K, N, max_seq_len, seed, spare=0):
    """jagged, bias, g ~ N(0, 1), dense ~ N(0, 1 / K) (outputs of O(1)); `spare` rows behind offsets[B] -> p"""
    gen = torch.Generator().manual_seed(seed)
    offsets = torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0)
    L, B = int(offsets[-1]) + spare, len(lengths)
    return {"offsets": offsets, "max_seq_len": max_seq_len, "jagged": torch.randn(L, K, generator=gen),
            "dense": torch.randn(B, K, N, generator=gen) * K ** -0.5, "bias": torch.randn(B, N, generator=gen), "g": torch.randn(L, N, generator=gen)}


def gaps(p, want64, dtype=torch.float32):
    lit = literal(p, dtype)
    return {k: rel_err(lit[k], want64[k]) for k in KINDS}
