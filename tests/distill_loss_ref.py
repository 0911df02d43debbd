"""Restatement of Rocket Launching's distillation terms for the tests (tzrec/models/rocket_launching.py:125-155, 182-215), in
plain torch on the CPU in the dtype asked for: the loss weight w / mean(w) (0 where the mean is 0); per pair of hidden layers
either -0.1 mean(sum(normalize(booster) normalize(light), 1) lw) or sqrt(sum(sum((booster - light)^2, 1) lw)), the booster
detached; the hint MSELoss(light logits, booster logits), per element and then mean(hint lw) with weights; gradients by autograd
for the upstream gradients `upstream(P)`.  In float64 it is the truth the kernel is held to; in float32 it is the yardstick
(`gap`): the literal form's own distance to float64 on the same inputs.  Nothing here touches the package under test."""
import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)


def kinds(P):
    """every output its own kind: sim_p, hint, d light_p, d logits_light"""
    return [f"sim{p}" for p in range(P)] + ["hint"] + [f"dl{p}" for p in range(P)] + ["dll"]


def upstream(P):
    """distinct per term, none of them 1: (sim_0 .. sim_{P-1}, hint)"""
    return [0.37 - 0.21 * p for p in range(P)] + [-2.0]


def literal(ls, bs, ll, lb, cosine, w=None, g=None, dtype=torch.float64):
    """ls[p], bs[p] [B, W_p], ll, lb [B] or [B, C], w [B] or None -> kind -> [tensor]"""
    P = len(ls)
    g = upstream(P) if g is None else g
    ls = [t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in ls]
    bs = [t.detach().cpu().to(dtype) for t in bs]
    ll = ll.detach().cpu().to(dtype).clone().requires_grad_(True)
    lb = lb.detach().cpu().to(dtype)
    lw = None
    if w is not None:
        w = w.detach().cpu().to(dtype)
        den = torch.mean(w)
        lw = w / den if float(den) != 0.0 else torch.zeros_like(w)
    sims = []
    for l, b in zip(ls, bs):
        if cosine:
            rows = torch.sum(torch.mul(F.normalize(b, p=2, dim=1), F.normalize(l, p=2, dim=1)), dim=1)
            sims.append(-0.1 * torch.mean(rows * lw if lw is not None else rows))
        else:
            sq = torch.square(b - l)
            if lw is not None:
                sq = torch.sum(sq, dim=1) * lw
            sims.append(torch.sqrt(torch.sum(sq)))
    if lw is not None:
        hint = torch.mean(F.mse_loss(ll, lb, reduction="none") * lw)
    else:
        hint = F.mse_loss(ll, lb)
    total = sum(t * c for t, c in zip(sims + [hint], g) if c is not None)
    grads = torch.autograd.grad(total, ls + [ll], allow_unused=True)
    grads = [torch.zeros_like(t) if d is None else d for d, t in zip(grads, ls + [ll])]
    out = {f"sim{p}": [sims[p].detach()] for p in range(P)}
    out["hint"] = [hint.detach()]
    out.update({f"dl{p}": [grads[p]] for p in range(P)})
    out["dll"] = [grads[P]]
    return out


def gaps(ls, bs, ll, lb, cosine, w, g, want64):
    r32 = literal(ls, bs, ll, lb, cosine, w, g, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in want64}


def draw(B, widths, C, seed, weights=None):
    """light rows ~ N(0, 1) scaled per row by a factor in [0.25, 4) (the norms differ), booster rows ~ N(0, 1), logits ~ N(0, 1)
    ([B] when C is 1, as the squeezed BCE logits are); weights: None, "rand" (uniform [0.5, 1.5)) or "zero" -> ls, bs, ll, lb, w
    (CPU tensors)"""
    g = torch.Generator().manual_seed(seed)
    ls = [torch.randn(B, W, generator=g) * 2.0 ** (torch.rand(B, 1, generator=g) * 4 - 2) for W in widths]
    bs = [torch.randn(B, W, generator=g) for W in widths]
    shape = (B,) if C == 1 else (B, C)
    ll, lb = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    w = None if weights is None else (torch.zeros(B) if weights == "zero" else 0.5 + torch.rand(B, generator=g))
    return ls, bs, ll, lb, w
