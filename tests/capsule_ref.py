"""Restatement of MIND's capsule layer for the tests (tzrec/modules/capsule.py:105-231), in plain torch on the CPU in the dtype
asked for: pad / truncate the jagged rows to [B, S, L], sequence and capsule masks (the capsule count by the reference's float
log2 form), the detached routing rounds, squash, gradients by autograd against a fixed upstream gradient.  In float64 it is the
truth the kernel is held to; in float32 it is the yardstick (`gaps`): the literal form's own distance to float64 on the same
inputs -- the larger of two evaluations, as given and with each sample's positions reversed (routing is equivariant under
that permutation; the softmax at scale 20 saturates and one fp32 run is a noisy estimate of its sensitivity).  Nothing here
touches the package under test."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

KINDS = ("high", "c", "dX", "dW")
C_YARDSTICK_MAX = 2.0 ** -12  # a draw whose literal fp32 routing weights are further from float64 amplifies a near-tie
SETTINGS = {
    "scale1_std0.1_pow2": dict(routing_logits_scale=1.0, routing_logits_stddev=0.1, squash_pow=2.0),  # the reference test's
    "scale20_std1_pow1": dict(routing_logits_scale=20.0, routing_logits_stddev=1.0, squash_pow=1.0),  # the defaults
}


def config(S=20, K=4, H=8, iters=3, const_caps_num=False, init="zeros", **setting):
    base = dict(routing_logits_scale=20.0, routing_logits_stddev=1.0, squash_pow=1.0)
    base.update(setting)
    return SimpleNamespace(max_seq_len=S, max_k=K, high_dim=H, num_iters=iters, const_caps_num=const_caps_num, routing_init_method=init, **base)


def offsets_of(lengths):
    return torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0)


def integer_mask(lengths, K, const_caps_num):
    """k_b = max(1, #{ j < K : 2^j < len_b }) -> bool [B, K]"""
    rows = []
    for n in lengths:
        kb = K if const_caps_num else max(1, sum(1 for j in range(K) if 2 ** j < n))
        rows.append([k < kb for k in range(K)])
    return torch.tensor(rows, dtype=torch.bool).reshape(len(lengths), K)


def _squash(x, p):
    norm = torch.linalg.norm(x, dim=-1, keepdim=True)
    eps = torch.max(norm, torch.tensor(1e-7, dtype=x.dtype))
    return torch.pow(torch.square(eps) / (1 + torch.square(eps)), p) / eps * x


def literal(x, offsets, W, cfg, logits0, g, dtype=torch.float64, perm=None):
    """x [N, L], offsets [B + 1], W [L, H], logits0 [N, K] or None, g [B, K, H] the upstream gradient of `high` -> kind -> [tensor]
    (high [B, K, H], c [N, K], dX [N, L], dW [L, H]) and "mask" -> bool [B, K].  perm [N]: evaluate on the rows x[perm] (a
    permutation inside each sample) and hand c and dX back in the given order."""
    N, L = x.shape
    S, K = cfg.max_seq_len, cfg.max_k
    lx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    lw = W.detach().cpu().to(dtype).clone().requires_grad_(True)
    offsets = offsets.cpu()
    rows = lx if perm is None else lx[perm]
    l0 = None if logits0 is None else (logits0.detach().cpu().to(dtype) if perm is None else logits0.detach().cpu().to(dtype)[perm])
    seq_len = offsets[1:] - offsets[:-1]
    pos = torch.arange(S)
    seq_mask = pos[None, :] < seq_len[:, None]
    idx = torch.where(seq_mask, offsets[:-1, None] + pos[None, :], torch.full((1, S), N, dtype=torch.int64))
    sm = seq_mask.to(dtype)
    inputs = torch.cat([rows, torch.zeros(1, L, dtype=dtype)])[idx] * sm.unsqueeze(-1)
    if cfg.const_caps_num:
        n_high = torch.zeros_like(seq_len, dtype=torch.float32) + K
    else:
        n_high = torch.maximum(torch.Tensor([1]), torch.minimum(torch.Tensor([K]), torch.log2(seq_len.float())))
    capsule_mask = torch.arange(K)[None, :] < n_high[:, None]
    logits = torch.zeros(idx.shape + (K,), dtype=dtype) if l0 is None else torch.cat([l0, torch.zeros(1, K, dtype=dtype)])[idx]
    logits = logits.detach() * cfg.routing_logits_stddev
    thresh = (capsule_mask.unsqueeze(1).to(dtype) * 2 - 1) * float("inf")
    low = torch.einsum("bsl, lh -> bsh", inputs, lw)
    low_d = low.detach()
    low_dn = F.normalize(low_d, p=2.0, dim=-1)
    for it in range(cfg.num_iters):
        logits = torch.minimum(logits, thresh)
        logits = F.softmax(logits * cfg.routing_logits_scale, dim=2)
        logits = logits * sm.unsqueeze(2)
        if it + 1 < cfg.num_iters:
            high = torch.einsum("bsh,bsk->bkh", low_d, logits)
            logits = logits + torch.einsum("bkh, bsh -> bsk", high, low_dn)
        else:
            high = _squash(torch.einsum("bsh,bsk->bkh", low, logits), cfg.squash_pow)
    high = high * capsule_mask.unsqueeze(-1).to(dtype)
    dx, dw = torch.autograd.grad((high * g.detach().cpu().to(dtype)).sum(), [lx, lw], allow_unused=True)
    dx = torch.zeros_like(lx) if dx is None else dx
    c_rows = torch.zeros(N + 1, K, dtype=dtype)
    c_rows[idx.reshape(-1)] = logits.detach().reshape(-1, K)  # (padded positions land in the spare row N; rows behind S stay 0)
    c = c_rows[:N]
    if perm is not None:
        back = torch.empty_like(c)
        back[perm] = c
        c = back
    return {"high": [high.detach()], "c": [c], "dX": [dx], "dW": [dw], "mask": capsule_mask}


def reversal(offsets, S):
    """the permutation that reverses each sample's first min(len, S) rows"""
    offsets = offsets.tolist()
    perm = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        s = min(b - a, S)
        perm += list(range(a + s - 1, a - 1, -1)) + list(range(a + s, b))
    return torch.tensor(perm, dtype=torch.int64)


def gaps(x, offsets, W, cfg, logits0, g, want64):
    r32 = literal(x, offsets, W, cfg, logits0, g, torch.float32)
    p32 = literal(x, offsets, W, cfg, logits0, g, torch.float32, perm=reversal(offsets, cfg.max_seq_len))
    out = {k: max(rel_err(r32[k], want64[k]), rel_err(p32[k], want64[k])) for k in KINDS}
    assert out["c"] < C_YARDSTICK_MAX, f"the draw amplifies a near-tie: literal fp32 c is {out['c']:.3e} from float64"
    return out


def draw(lengths, L, H, K, seed, with_logits0=True):
    """x ~ 0.5 N(0, 1) [N, L], W ~ N(0, 1) [L, H], logits0 ~ N(0, 1) [N, K] (or None), g ~ N(0, 1) [B, K, H] -> offsets, x, W, logits0, g"""
    gen = torch.Generator().manual_seed(seed)
    offsets = offsets_of(lengths)
    N = int(offsets[-1])
    x = 0.5 * torch.randn(N, L, generator=gen)
    W = torch.randn(L, H, generator=gen)
    l0 = torch.randn(N, K, generator=gen)
    g = torch.randn(len(lengths), K, H, generator=gen)
    return offsets, x, W, (l0 if with_logits0 else None), g


# ---- label-aware attention (tzrec/models/mind.py:303-333) ----------------------------------------------------------------------
LA_KINDS = ("user_emb", "w", "dI", "dV")


def la_literal(interests, item, mask, simi_pow, g, dtype=torch.float64):
    """interests [B, K, D], item [M, D], mask [B, K] bool, g [B, D] the upstream gradient -> kind -> [tensor] (user_emb [B, D], w [B, K],
    dI [B, K, D], dV [M, D])"""
    li = interests.detach().cpu().to(dtype).clone().requires_grad_(True)
    lv = item.detach().cpu().to(dtype).clone().requires_grad_(True)
    mask = mask.cpu()
    weight = torch.einsum("bkd, bd->bk", li, lv[:li.size(0)])
    weight = torch.minimum(weight, (mask.to(dtype) * 2 - 1) * float("inf"))
    weight = F.softmax(weight.unsqueeze(-1) * simi_pow, dim=1)
    emb = torch.sum(torch.multiply(weight, li), dim=1)
    di, dv = torch.autograd.grad((emb * g.detach().cpu().to(dtype)).sum(), [li, lv])
    return {"user_emb": [emb.detach()], "w": [weight.detach().squeeze(-1)], "dI": [di], "dV": [dv]}


def la_gaps(interests, item, mask, simi_pow, g, want64):
    r32 = la_literal(interests, item, mask, simi_pow, g, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in LA_KINDS}


def la_draw(B, K, D, M, valid, seed):
    """interests, item ~ N(0, 1) D^-1/4 (dots of order 1), g ~ N(0, 1); valid: "one", "some" (k_b uniform in 1..K) or "all" -> prefix masks"""
    gen = torch.Generator().manual_seed(seed)
    interests, item = torch.randn(B, K, D, generator=gen) * D ** -0.25, torch.randn(M, D, generator=gen) * D ** -0.25
    g = torch.randn(B, D, generator=gen)
    kb = {"one": torch.ones(B, dtype=torch.int64), "all": torch.full((B,), K), "some": torch.randint(1, K + 1, (B,), generator=gen)}[valid]
    return interests, item, torch.arange(K)[None, :] < kb[:, None], g
