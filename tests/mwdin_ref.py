"""Restatement of TDM's multi-window DIN encoder for the tests (tzrec/modules/sequence.py:330-367), in plain torch on the CPU in the
dtype asked for: pad the jagged rows to [B, T, C], [k, q * k, q] -> layers -> linear -> PReLU, mask, negative pad, torch.segment_reduce,
the divide by the lengths as handed over (NOT truncated to T), gradients by autograd against a fixed upstream gradient.  In float64 it
is the truth the kernel is held to; in float32 the yardstick (`gaps`).  Nothing here touches the package under test."""
import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

KINDS = ("out", "dK", "dQ", "dW", "db", "dw3", "db3", "dslope", "dalpha")
KINK = 1e-4  # no float64 pre-activation and no a_n of a position that takes part lies closer to zero: no kink flips in fp32


def literal(p, dtype=torch.float64):
    """p: what `draw` returns -> kind -> [tensors], and "margin": the smallest |pre-activation| / |a_n| among the positions < min(len, T)"""
    c = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)  # noqa: E731
    x, q, w3, b3, alpha = c(p["x"]), c(p["q"]), c(p["w3"]), c(p["b3"]), c(p["alpha"])
    Ws, bs, sl = [c(w) for w in p["W"]], [c(b) for b in p["b"]], [None if s is None else c(s) for s in p["slope"]]
    offsets, T, (N, C) = p["offsets"], p["T"], x.shape
    lens = offsets[1:] - offsets[:-1]
    pos = torch.arange(T)
    mask = pos[None, :] < lens[:, None]
    idx = torch.where(mask, offsets[:-1, None] + pos[None, :], torch.full((1, T), N, dtype=torch.int64))
    seq = torch.cat([x, torch.zeros(1, C, dtype=dtype)])[idx]  # [B, T, C]
    query = F.pad(q, (0, C - q.shape[1]))
    qs = query.unsqueeze(1).expand(-1, T, -1)
    h, margin = torch.cat([seq, qs * seq, qs], dim=-1), float("inf")
    for W, b, s in zip(Ws, bs, sl):
        z = F.linear(h, W, b)
        margin = min(margin, float(z.detach().abs()[mask].min()) if mask.any() else margin)
        h = F.relu(z) if s is None else F.prelu(z, s)
    a = F.linear(h, w3, b3)
    margin = min(margin, float(a.detach().abs()[mask].min()) if mask.any() else margin)
    att = F.prelu(a, alpha) * mask.unsqueeze(2) * seq
    wl = torch.tensor(p["windows"])
    cum = torch.cumsum(wl, 0) - wl
    res = torch.segment_reduce(F.pad(att, (0, 0, 0, int(wl.sum()) - T)).transpose(0, 1), reduce="sum", lengths=wl, axis=0).transpose(0, 1)
    seg = torch.min(lens.unsqueeze(1) - cum.unsqueeze(0), wl)
    out = torch.cat([res / torch.max(seg, torch.ones_like(seg)).unsqueeze(2), query.unsqueeze(1)], dim=1).reshape(len(lens), -1)
    leaves = [x, q, *Ws, *bs, w3, b3, *[s for s in sl if s is not None], alpha]
    gr = list(torch.autograd.grad((out * p["g"].to(dtype)).sum(), leaves, allow_unused=True))
    gr = [torch.zeros_like(t) if g is None else g for g, t in zip(gr, leaves)]
    nl = len(Ws)
    return {"out": [out.detach()], "dK": [gr[0]], "dQ": [gr[1]], "dW": gr[2:2 + nl], "db": gr[2 + nl:2 + 2 * nl], "dw3": [gr[2 + 2 * nl]],
            "db3": [gr[3 + 2 * nl]], "dslope": gr[4 + 2 * nl:-1], "dalpha": [gr[-1]], "margin": margin}


def draw(lengths, windows, T, C, hidden, prelu, seed, Dq=None):
    """rows ~ 0.5 N(0, 1), query ~ N(0, 1), layers ~ N(0, 1) / sqrt(fan in), slopes 0.25 (PReLU's own start), g ~ N(0, 1); the seed steps
    by 1000 until the float64 form keeps every kink at KINK (a condition on the inputs, checked with the reference alone)"""
    for n in range(16):
        gen = torch.Generator().manual_seed(seed + 1000 * n)
        r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        offsets = torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0)
        p = {"offsets": offsets, "windows": list(windows), "T": T, "x": 0.5 * r(int(offsets[-1]), C), "q": r(len(lengths), Dq or C), "W": [], "b": [],
             "slope": [], "alpha": torch.tensor([0.25]), "g": r(len(lengths), (len(windows) + 1) * C)}
        d = 3 * C
        for h in hidden:
            p["W"].append(r(h, d) / d ** 0.5), p["b"].append(0.5 * r(h)), p["slope"].append(torch.tensor([0.25]) if prelu else None)
            d = h
        p["w3"], p["b3"] = r(1, d) / d ** 0.5, 0.5 * r(1)
        want = literal(p)
        if want["margin"] >= KINK:
            return p, want
    raise AssertionError("no draw keeps its kinks away from zero")


def gaps(p, want64):
    r32 = literal(p, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in KINDS}
