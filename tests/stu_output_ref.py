"""Restatement of the STU layer's output stage for the tests (the formulas and the keep rule of include/tzrec_hip.h, TzrStuOutput):
plain torch on the CPU in the dtype asked for, gradients by autograd against a fixed upstream gradient.  In float64 it is the
truth the kernels are held to, in float32 the yardstick (`gaps`).  Nothing here touches the package under test."""
import numpy as np
import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

KINDS = ("out", "du", "dattn", "dx", "dWo", "dgamma", "dbeta")
LEAVES = ("u", "attn", "x", "wo", "gamma", "beta")
G = 0x9E3779B97F4A7C15


def keep(L, W, p, seed):
    """bool [L, 3 W], integer by integer (uint64 arithmetic wraps)"""
    z = np.uint64(seed % 2 ** 64) + np.arange(1, L * 3 * W + 1, dtype=np.uint64) * np.uint64(G) + np.uint64(G)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return torch.from_numpy(((z >> np.uint64(40)) >= np.uint64(int(float(np.float32(p)) * 2 ** 24))).reshape(L, 3 * W))


def literal(c, dtype=torch.float64):
    """c: the operands (u the RAW slice), H, group_norm, p, training, seed, eps, g -> kind -> [tensor]"""
    u, attn, x, wo, gamma, beta = (c[k].detach().to(dtype).clone().requires_grad_(True) for k in LEAVES)
    (L, W), H = u.shape, c["H"]
    us = F.silu(u)
    a = attn.view(L, H, W // H) if c["group_norm"] else attn.view(L, 1, W)
    nh = (a - a.mean(2, keepdim=True)) * torch.rsqrt(a.var(2, unbiased=False, keepdim=True) + c["eps"])
    n = nh * gamma.view(1, H, 1) + beta.view(1, H, 1) if c["group_norm"] else nh * gamma + beta
    C = torch.cat([us, attn, us * n.reshape(L, W)], dim=1)
    if c["training"] and c["p"] > 0:
        C = C * keep(L, W, c["p"], c["seed"]).to(dtype) / (1.0 - c["p"])
    out = x + C @ wo
    grads = torch.autograd.grad((out * c["g"].to(dtype)).sum(), [u, attn, x, wo, gamma, beta])
    return dict(zip(KINDS, [[out.detach()]] + [[t] for t in grads]))


def draw(L, E, H, Dv, group_norm, p, seed, training=True):
    """u the first W columns of a wider matrix as the layer's uvqk product leaves it, every parameter off its constant start"""
    gen, W = torch.Generator().manual_seed(seed), H * Dv
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    n = H if group_norm else W
    wide = r(L, 2 * W + 8)
    c = {"wide": wide, "u": wide[:, :W], "attn": r(L, W), "x": r(L, E), "wo": r(3 * W, E) / (3 * W) ** 0.5, "gamma": 1.0 + 0.2 * r(n),
         "beta": 0.2 * r(n), "g": r(L, E), "H": H, "group_norm": group_norm, "p": p, "training": training, "seed": 1_000_003 * (seed + 1), "eps": 1e-6}
    want, r32 = literal(c), literal(c, torch.float32)
    return c, want, {k: rel_err(r32[k], want[k]) for k in KINDS}
