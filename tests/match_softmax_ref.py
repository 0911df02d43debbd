"""Restatement of the match models' similarity head for the tests (tzrec/models/match_model.py:50-64, 303-336, dssm.py:81-83,
147-155), in plain torch on the CPU in the dtype asked for: F.normalize, the positive's multiply-and-sum, the negatives' matmul,
the cat, the division by the temperature, CrossEntropyLoss (with sample weights mean(l w) / mean(w), 0 where mean(w) is 0);
gradients by autograd.  In float64 it is the truth the kernel is held to; in float32 it is the yardstick (`gap`): the literal
form's own distance to float64 on the same inputs.  Nothing here touches the package under test.

`rank` (the number of other columns strictly above the positive's score) is compared EXACTLY, so `draw` steps its seed until the
inputs are settled: no other column's float64 score within RANK_MARGIN of its row's positive, where fp32 could take the other
side -- a condition on the inputs, checked with the reference alone."""
import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

SAMPLED, IN_BATCH = 0, 1
KINDS = ("loss", "lse", "dU", "dV", "sim")
RANK_MARGIN = 2.0 ** -14
MAX_DRAWS = 8


def scores(u, v, mode, cosine, T):
    if cosine:
        u, v = F.normalize(u, p=2.0, dim=1), F.normalize(v, p=2.0, dim=1)
    if mode == IN_BATCH:
        return torch.mm(u, v.T) / T
    B = u.shape[0]
    pos = torch.sum(u * v[:B], dim=-1, keepdim=True)
    return torch.cat([pos, torch.matmul(u, v[B:].T)], dim=-1) / T


def labels(B, mode):
    return torch.arange(B) if mode == IN_BATCH else torch.zeros(B, dtype=torch.long)


def literal(u, v, mode, cosine, T, w=None, dtype=torch.float64):
    """-> kind -> [tensor] (loss, lse, dU, dV, sim) and "rank" -> int32 [B]"""
    lu = u.detach().cpu().to(dtype).clone().requires_grad_(True)
    lv = v.detach().cpu().to(dtype).clone().requires_grad_(True)
    sim = scores(lu, lv, mode, cosine, T)
    y = labels(lu.shape[0], mode)
    if w is None:
        loss = F.cross_entropy(sim, y)
    else:
        lw = w.detach().cpu().to(dtype)
        num, den = torch.mean(F.cross_entropy(sim, y, reduction="none") * lw), torch.mean(lw)
        loss = num / den if float(den) != 0.0 else num * 0.0
    du, dv = torch.autograd.grad(loss, [lu, lv])
    pos = sim.detach().gather(1, y[:, None])
    return {"loss": [loss.detach()], "lse": [torch.logsumexp(sim.detach(), dim=1)], "dU": [du], "dV": [dv], "sim": [sim.detach()],
            "rank": (sim.detach() > pos).sum(dim=1).to(torch.int32)}


def gaps(u, v, mode, cosine, T, w, want64):
    r32 = literal(u, v, mode, cosine, T, w, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in KINDS}


def min_rank_gap(u, v, mode, cosine, T):
    """the smallest float64 |s_ij - s_i,label| over the columns j != label (inf without such a column)"""
    sim = scores(u.double(), v.double(), mode, cosine, T)
    y = labels(u.shape[0], mode)
    d = (sim - sim.gather(1, y[:, None])).abs()
    d.scatter_(1, y[:, None], float("inf"))
    return float(d.min()) if d.numel() else float("inf")


def draw(B, N, D, mode, cosine, T, seed, weights=None):
    """u [B, D], v [M, D] ~ N(0, 1) (inner product: scaled by D^-1/4 so that the scores are of order 1), M = B + N (SAMPLED) or B;
    weights: None, "rand" (uniform (0, 2)) or "zero" -> u, v, w (CPU tensors).  The seed steps by 1000 until the draw is settled;
    at most MAX_DRAWS draws."""
    M = B + N if mode == SAMPLED else B
    for n in range(MAX_DRAWS):
        g = torch.Generator().manual_seed(seed + 1000 * n)
        scale = 1.0 if cosine else D ** -0.25
        u, v = torch.randn(B, D, generator=g) * scale, torch.randn(M, D, generator=g) * scale
        w = None if weights is None else (torch.zeros(B) if weights == "zero" else torch.rand(B, generator=g) * 2)
        if min_rank_gap(u, v, mode, cosine, T) >= RANK_MARGIN:
            return u, v, w
    raise AssertionError(f"no settled draw within {MAX_DRAWS} draws at B{B} N{N} D{D}")
