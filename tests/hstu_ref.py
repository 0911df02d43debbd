"""Restatement of HSTU's jagged attention for the tests: per sample and head the dense form of
    out[i] = sum_j valid(i, j) silu(alpha <q_i, k_j>) / scale v_j        over the n = min(len, max_seq_len) rows a sample keeps,
in plain torch on the CPU in the dtype asked for, the mask built entry by entry from the index rule of include/tzrec_hip.h,
gradients by autograd against a fixed upstream gradient.  In float64 it is the truth the kernels are held to; in float32 the
yardstick (`gaps`).  Nothing here touches the package under test."""
import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

KINDS = ("out", "dq", "dk", "dv")


def valid_mask(n, t, c, L):
    """bool [n, n]; t None: num_targets not given"""
    def ident(i):
        v = i if c == 0 else max(i - c + 1, 0)
        return v if t is None else min(v, max_id)

    max_id = (n if c == 0 else n - c + 1) - (t or 0)
    m = torch.zeros(n, n, dtype=torch.bool)
    for i in range(n):
        for j in range(n):
            d = ident(i) - ident(j)
            ok = i == j or d > 0
            if L > 0:
                ok = ok and d <= L
            if c > 0:
                ok = ok or (ident(i) == 0 and ident(j) < max_id)
            m[i, j] = ok
    return m


def attention(p, q, k, v, dtype=torch.float64):
    """q, k [N, H, Da], v [N, H, Dv] of `dtype` -> out [N, H, Dv]; rows behind max_seq_len stay zero"""
    scale = float(p["scaling_seqlen"] if p["scaling_seqlen"] > 0 else p["max_seq_len"])
    outs, offsets = [], p["offsets"].tolist()
    for b in range(len(offsets) - 1):
        s, ln = offsets[b], offsets[b + 1] - offsets[b]
        n = min(ln, p["max_seq_len"])
        t = None if p["num_targets"] is None else int(p["num_targets"][b])
        mask = valid_mask(n, t, p["c"], p["L"]).to(dtype)
        a = F.silu(torch.einsum("xha,yha->hxy", q[s:s + n], k[s:s + n]) * p["alpha"]) / scale * mask
        outs += [torch.einsum("hxy,yhv->xhv", a, v[s:s + n]), v.new_zeros(ln - n, v.shape[1], v.shape[2])]
    return torch.cat(outs + [v[:0]])  # (an empty batch still hangs on v: autograd has a graph to walk)


def literal(p, dtype=torch.float64):
    q, k, v = (p[x].detach().to(dtype).clone().requires_grad_(True) for x in "qkv")
    out = attention(p, q, k, v, dtype)
    dq, dk, dv = torch.autograd.grad((out * p["g"].to(dtype)).sum(), [q, k, v], allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g  # noqa: E731
    return {"out": [out.detach()], "dq": [z(dq, q)], "dk": [z(dk, k)], "dv": [z(dv, v)]}


def draw(lengths, H, Da, Dv, max_seq_len, seed, num_targets=None, L=0, c=0, scaling_seqlen=-1):
    """q, k ~ N(0, 1) (alpha = Da^-1/2 keeps the scores O(1)), v, g ~ N(0, 1) -> p, and the float64 truth"""
    gen = torch.Generator().manual_seed(seed)
    offsets = torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0)
    N = int(offsets[-1])
    p = {"offsets": offsets, "max_seq_len": max_seq_len, "alpha": Da ** -0.5, "L": L, "c": c, "scaling_seqlen": scaling_seqlen,
         "num_targets": None if num_targets is None else torch.tensor(num_targets, dtype=torch.int64),
         "q": torch.randn(N, H, Da, generator=gen), "k": torch.randn(N, H, Da, generator=gen), "v": torch.randn(N, H, Dv, generator=gen),
         "g": torch.randn(N, H, Dv, generator=gen)}
    return p, literal(p)


def gaps(p, want64):
    r32 = literal(p, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in KINDS}
