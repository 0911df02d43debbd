"""Restatement of the low-rank cross network of Deep & Cross v2 for the tests (tzrec/modules/interaction.py:167-180), in plain
torch on the CPU in the dtype asked for: the literal loop `x_l = x_0 * v_i(u_i(x_l)) + x_l` and its autograd.  In float64 it
is the truth the kernels are held to; in float32 it is the yardstick (`gap`): the literal form's own distance to float64 on
the same inputs.  Nothing here touches the package under test."""
import torch

KINDS = ("y", "gx", "gu", "gv", "gc")
FLOOR = 2.0 ** -20  # 8 ulp of 1.0: guards the degenerate cases whose gap can land near zero by chance


def literal(x, us, vs, cs, gy, dtype=torch.float64):
    """x [B, D], us: L tensors [r, D], vs: L tensors [D, r], cs: L tensors [D], gy [B, D] ->
    {"y": [y], "gx": [gx], "gu": [...], "gv": [...], "gc": [...]}"""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    us, vs, cs = ([p.detach().cpu().to(dtype).clone().requires_grad_(True) for p in ps] for ps in (us, vs, cs))
    x_l = x
    for u, v, c in zip(us, vs, cs):
        x_l = x * torch.nn.functional.linear(torch.nn.functional.linear(x_l, u), v, c) + x_l
    if us:
        x_l.backward(gy.detach().cpu().to(dtype))
        gx = x.grad
    else:
        gx = gy.detach().cpu().to(dtype)
    return {"y": [x_l.detach()], "gx": [gx], "gu": [p.grad for p in us], "gv": [p.grad for p in vs], "gc": [p.grad for p in cs]}


def rel_err(got, want64):
    """max |got - fp64| / max(1, |fp64|) over the tensors of one kind"""
    err = 0.0
    for a, e in zip(got, want64):
        a = a.detach().cpu().to(torch.float64).reshape(e.shape)
        if e.numel():
            err = max(err, float(((a - e).abs() / e.abs().clamp(min=1.0)).max()))
    return err


def literal_gaps(x, us, vs, cs, gy, want64):
    """per kind: the fp32 literal form's distance to the float64 evaluation of the same inputs"""
    r32 = literal(x, us, vs, cs, gy, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in KINDS}


def check(got, want64, gaps, what):
    """every kind within max(4 x gap, 2^-20); prints each figure (and ours / literal) before it asserts"""
    bad = []
    for k in KINDS:
        err, bound = rel_err(got[k], want64[k]), max(4.0 * gaps[k], FLOOR)
        print(f"{what} {k}: err {err:.3e} gap {gaps[k]:.3e} ours/literal {err / gaps[k] if gaps[k] else float('inf'):.2f} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, f"{what}: {bad}"


def draw(B, D, R, L, seed):
    """x ~ 0.5 N(0,1); u, v and c uniform within nn.Linear's default bounds (1 / sqrt(fan_in)); gy ~ N(0,1)"""
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(B, D, generator=g)
    us = [(torch.rand(R, D, generator=g) * 2 - 1) / D ** 0.5 for _ in range(L)]
    vs = [(torch.rand(D, R, generator=g) * 2 - 1) / R ** 0.5 for _ in range(L)]
    cs = [(torch.rand(D, generator=g) * 2 - 1) / R ** 0.5 for _ in range(L)]
    gy = torch.randn(B, D, generator=g)
    return x, us, vs, cs, gy
