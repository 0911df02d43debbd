"""Restatement of DAT's Adaptive-Mimic loss for the tests (tzrec/models/dat.py:100-101, 206-207, 212-259), in plain torch on the
CPU in the dtype asked for: the towers' embeddings detached and, under COSINE, normalized; per side F.normalize of the augment
rows, the slice to the batch, subtract, square, sum (over everything, or per row with sample weights: then mean(l w) / mean(w), 0
where mean(w) is 0); gradients by autograd for the upstream gradients (g_u, g_i).  In float64 it is the truth the kernel is held to;
in float32 it is the yardstick (`gap`): the literal form's own distance to float64 on the same inputs.  Nothing here touches the
package under test."""
import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

KINDS = ("loss_u", "loss_i", "dA_u", "dA_i")
UPSTREAM = (0.37, -2.0)


def literal(ua, ia, ue, ie, cosine, c_u, c_i, w=None, g=UPSTREAM, dtype=torch.float64):
    """ua [B, D], ia [M, D], ue [B, D], ie [M, D] -> kind -> [tensor]; dA_i is [M, D] (zero rows behind B)"""
    ua = ua.detach().cpu().to(dtype).clone().requires_grad_(True)
    ia = ia.detach().cpu().to(dtype).clone().requires_grad_(True)
    ue, ie = ue.detach().cpu().to(dtype), ie.detach().cpu().to(dtype)
    if cosine:
        ue, ie = F.normalize(ue, p=2.0, dim=1), F.normalize(ie, p=2.0, dim=1)
    B = ua.size(0)
    dim = 1 if w is not None else (0, 1)
    lu = c_u * torch.sum(torch.square(F.normalize(ua, p=2.0, dim=1) - ie[:B]), dim=dim)
    li = c_i * torch.sum(torch.square(F.normalize(ia[:B], p=2.0, dim=1) - ue), dim=dim)
    if w is not None:
        lw = w.detach().cpu().to(dtype)
        den = torch.mean(lw)
        lu, li = (torch.mean(l * lw) / den if float(den) != 0.0 else torch.mean(l * lw) * 0.0 for l in (lu, li))
    du, di = torch.autograd.grad(lu * g[0] + li * g[1], [ua, ia])
    return {"loss_u": [lu.detach()], "loss_i": [li.detach()], "dA_u": [du], "dA_i": [di]}


def gaps(ua, ia, ue, ie, cosine, c_u, c_i, w, g, want64):
    r32 = literal(ua, ia, ue, ie, cosine, c_u, c_i, w, g, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in KINDS}


def draw(B, M, D, seed, weights=None):
    """augment rows ~ N(0, 1) scaled per row by a factor in [0.25, 4) (the norms differ), embeddings ~ N(0, 1) D^-1/2 (of order one
    without the normalisation); weights: None, "rand" (uniform [0.5, 1.5)) or "zero" -> ua, ia, ue, ie, w (CPU tensors)"""
    g = torch.Generator().manual_seed(seed)
    scale = lambda n: 2.0 ** (torch.rand(n, 1, generator=g) * 4 - 2)  # noqa: E731
    ua, ia = torch.randn(B, D, generator=g) * scale(B), torch.randn(M, D, generator=g) * scale(M)
    ue, ie = torch.randn(B, D, generator=g) * D ** -0.5, torch.randn(M, D, generator=g) * D ** -0.5
    w = None if weights is None else (torch.zeros(B) if weights == "zero" else 0.5 + torch.rand(B, generator=g))
    return ua, ia, ue, ie, w
