"""Restatement of the cross network of Deep & Cross v1 for the tests (tzrec/modules/interaction.py:126-132), in plain torch
on the CPU in the dtype asked for: the literal loop `x1 = w_i(x1) * x + b_i + x1` and its autograd.  In float64 it is the
truth the kernels are held to; in float32 it is the yardstick (`gap`): the literal form's own distance to float64 on the
same inputs.  Nothing here touches the package under test."""
import torch

KINDS = ("y", "gx", "gw", "gb")
FLOOR = 2.0 ** -20  # 8 ulp of 1.0: guards the degenerate cases whose gap can land near zero by chance


def cross_literal(x, ws, bs, gy, dtype=torch.float64):
    """x [B, D], ws: L tensors [1, D], bs: L tensors [D], gy [B, D] -> {"y": [y], "gx": [gx], "gw": [...], "gb": [...]}"""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    ws = [w.detach().cpu().to(dtype).clone().requires_grad_(True) for w in ws]
    bs = [b.detach().cpu().to(dtype).clone().requires_grad_(True) for b in bs]
    x1 = x
    for w, b in zip(ws, bs):
        x1 = torch.nn.functional.linear(x1, w) * x + b + x1
    if ws:
        x1.backward(gy.detach().cpu().to(dtype))
        gx = x.grad
    else:
        gx = gy.detach().cpu().to(dtype)
    return {"y": [x1.detach()], "gx": [gx], "gw": [w.grad for w in ws], "gb": [b.grad for b in bs]}


def rel_err(got, want64):
    """max |got - fp64| / max(1, |fp64|) over the tensors of one kind"""
    err = 0.0
    for a, e in zip(got, want64):
        a = a.detach().cpu().to(torch.float64).reshape(e.shape)
        if e.numel():
            err = max(err, float(((a - e).abs() / e.abs().clamp(min=1.0)).max()))
    return err


def literal_gaps(x, ws, bs, gy, want64):
    """per kind: the fp32 literal form's distance to the float64 evaluation of the same inputs"""
    r32 = cross_literal(x, ws, bs, gy, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in KINDS}


def check(got, want64, gaps, what):
    """every kind within max(4 x gap, 2^-20); prints each figure before it asserts"""
    bad = []
    for k in KINDS:
        err, bound = rel_err(got[k], want64[k]), max(4.0 * gaps[k], FLOOR)
        print(f"{what} {k}: err {err:.3e} gap {gaps[k]:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, f"{what}: {bad}"


def draw(B, D, L, seed):
    """x ~ 0.5 N(0,1), w xavier-uniform, b ~ 0.1 N(0,1), gy ~ N(0,1)"""
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(B, D, generator=g)
    bound = (6.0 / (D + 1)) ** 0.5  # nn.init.xavier_uniform_ on a [1, D] weight
    ws = [(torch.rand(1, D, generator=g) * 2 - 1) * bound for _ in range(L)]
    bs = [0.1 * torch.randn(D, generator=g) for _ in range(L)]
    gy = torch.randn(B, D, generator=g)
    return x, ws, bs, gy
