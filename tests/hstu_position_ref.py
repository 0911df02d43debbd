"""Restatement of HSTU's positional / timestamp encoder for the tests: the rule of include/tzrec_hip.h row by row, in plain torch on
the CPU.  The sums run in the dtype asked for (float64: the truth; float32, bfloat16: the yardstick); the bucket rule is fp32
arithmetic in every case, as the contract says.  Gradients by autograd under a fixed upstream g.  Timestamps are drawn from chosen
bucket values, so that no row sits near a bucket's edge (`draw` asserts it).  Nothing here touches the package under test."""
import math

import torch

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

MARGIN = 0.05


def pre_bucket(gap, fn, incr, T, dtype=torch.float32):
    """the value the rule truncates, before its clamp: fn(max(gap, 1e-6) / incr) for int64 gaps"""
    u = gap.to(dtype).clamp(min=1e-6) / incr
    return torch.log(u) if fn == "log" else torch.sqrt(u)


def buckets(gap, fn, incr, T):
    return ((pre_bucket(gap, fn, incr, T) / T).clamp(min=0, max=1) * T).int().tolist()


def indices(p, b):
    """the kept positions of sample b -> (first row, position-table rows, gaps to the query time)"""
    s, n = int(p["offsets"][b]), int(p["offsets"][b + 1] - p["offsets"][b])
    t = 0 if p["num_targets"] is None else int(p["num_targets"][b]) * (2 if p["interleave"] else 1)
    P, c, keep = p["pos"].shape[0], p["c"], range(min(n, p["max_seq_len"]))
    if p["ts"] is None:
        return s, [max(min(i, min(n - t, P - 1)), 0) for i in keep], None
    idx = [i if i < c else min(n - t - min(i, n - t) + c, P - 1) for i in keep]
    qt = p["timestamps"][s + n - 1] if p["query_time"] is None else p["query_time"][b]
    return s, idx, qt - p["timestamps"][s:s + len(idx)]


def literal(p, dtype=torch.float64):
    x, pos = (p[k].detach().to(dtype).clone().requires_grad_(True) for k in ("x", "pos"))
    ts = None if p["ts"] is None else p["ts"].detach().to(dtype).clone().requires_grad_(True)
    out = [x * p["alpha"]]  # (alpha x alone for the rows no sample keeps)
    add = torch.zeros_like(out[0])
    for b in range(p["offsets"].numel() - 1):
        s, idx, gap = indices(p, b)
        if idx:
            rows = pos[idx] if ts is None else pos[idx] + ts[buckets(gap, p["fn"], p["incr"], ts.shape[0] - 1)]
            add = add.index_put((torch.arange(s, s + len(idx)),), rows, accumulate=True)
    out = out[0] + add
    leaves = [x, pos] + ([] if ts is None else [ts])
    grads = torch.autograd.grad((out * p["g"].to(dtype)).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    return {k: [t.detach()] for k, t in zip(("out", "dx", "dpos", "dts"), [out] + grads)}


def draw(lengths, E, P, T, max_seq_len, seed, num_targets=None, interleave=False, c=0, fn="sqrt", incr=60.0, given_query=False,
         equal=False, exact=True):
    """x, g ~ N(0, 1), tables within the encoder's initial bounds.  T None: the positional op.  Each row's timestamp is its
    sample's query time minus a gap whose bucket value was drawn: gap = round(incr f^-1(k + 1/2)).  `exact`: the second, third
    and fourth row of a sample get gap 0, a negative gap and a gap far past the last bucket; the last row always gets gap 0 (it is
    the default query time).  `equal`: every gap 0.  -> p"""
    gen = torch.Generator().manual_seed(seed)
    offsets = torch.tensor([0] + list(lengths), dtype=torch.int64).cumsum(0)
    L, B = int(offsets[-1]), len(lengths)
    p = {"offsets": offsets, "max_seq_len": max_seq_len, "alpha": E ** 0.5, "c": c, "interleave": interleave, "fn": fn, "incr": incr,
         "num_targets": None if num_targets is None else torch.tensor(num_targets, dtype=torch.int64),
         "x": torch.randn(L, E, generator=gen), "g": torch.randn(L, E, generator=gen),
         "pos": (torch.rand(P, E, generator=gen) * 2 - 1) * P ** -0.5, "ts": None, "timestamps": None, "query_time": None}
    if T is None:
        return p
    p["ts"] = (torch.rand(T + 1, E, generator=gen) * 2 - 1) * T ** -0.5
    k = torch.randint(0, T, (L,), generator=gen).double() + 0.5
    gap = (incr * (torch.exp(k) if fn == "log" else k * k)).round().to(torch.int64)
    for f in (torch.float32, torch.float64):  # the condition on the inputs: no drawn row within MARGIN of a bucket's edge
        v = pre_bucket(gap, fn, incr, T, f).double()
        assert bool(((v - v.round()).abs() >= MARGIN).all()) and bool((v < T).all()), "a drawn timestamp sits at a bucket's edge"
    far = int(incr * (math.exp(T + 3.0) if fn == "log" else (T + 3.0) ** 2))
    qt = 1_700_000_000 + 1000 * torch.arange(B, dtype=torch.int64)
    for b, n in enumerate(lengths):
        s = int(offsets[b])
        if exact:
            for i, v in ((1, 0), (2, -7), (3, far)):
                if i < n:
                    gap[s + i] = v
        if n:
            gap[s + n - 1] = 0
    if equal:
        gap.zero_()
    p["timestamps"] = qt.repeat_interleave(torch.tensor(list(lengths), dtype=torch.int64)) - gap if B else gap
    p["query_time"] = qt if given_query else None
    return p
