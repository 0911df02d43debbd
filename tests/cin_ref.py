"""Restatement of the compressed interaction network of xDeepFM for the tests (tzrec/modules/interaction.py:213-233), in plain
torch on the CPU in the dtype asked for, in two forms, both with autograd:

  literal    the reference's loop: z = einsum("bhd,bfd->bhfd"), reshape to [B, H F, D], conv1d(kernel_size=1), sum over d
  factored   f contracted first (u[b,o,h,d] = sum_f W[o,h,f] x0[b,f,d]), then h; the last layer's pooled output through the Gram
             matrix sum_d X^i[b,h,d] x0[b,f,d], so X^L is never formed

In float64 the literal form is the truth the kernels are held to.  In float32 the two forms are the yardstick (`gap`): a
kernel is free to associate either way, so the bound scales with the LARGER of the two forms' distances to float64 on the same
inputs.  Nothing here touches the package under test."""
import torch

KINDS = ("y", "gx", "gw", "gb")
FLOOR = 2.0 ** -20  # 8 ulp of 1.0: guards the degenerate cases whose gap can land near zero by chance


def _leaves(x, ws, bs, dtype):
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    ws = [w.detach().cpu().to(dtype).clone().requires_grad_(True) for w in ws]
    bs = [b.detach().cpu().to(dtype).clone().requires_grad_(True) for b in bs]
    return x, ws, bs


def _finish(y, x, ws, bs, gy):
    if x.shape[0] and ws:
        y.backward(gy.detach().cpu().to(y.dtype))
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)  # noqa: E731
    return {"y": [y.detach()], "gx": [zero(x)], "gw": [zero(w) for w in ws], "gb": [zero(b) for b in bs]}


def literal_forward(x, ws, bs):
    """the reference's loop on the tensors as they are (any device, any dtype): [B, F, D] -> [B, sum O]"""
    B, F, D = x.shape
    xv, outs = x, []
    for w, b in zip(ws, bs):
        z = torch.einsum("bhd,bfd->bhfd", xv, x).reshape(B, xv.shape[1] * F, D)
        xv = torch.nn.functional.conv1d(z, w, b)
        outs.append(xv.sum(dim=2))
    return torch.cat(outs, dim=1)


def factored_forward(x, ws, bs):
    B, F, D = x.shape
    xv, outs = x, []
    for i, (w, b) in enumerate(zip(ws, bs)):
        w3 = w.reshape(w.shape[0], xv.shape[1], F)
        if i == len(ws) - 1:
            gram = torch.einsum("bhd,bfd->bhf", xv, x)
            outs.append(torch.einsum("ohf,bhf->bo", w3, gram) + D * b)
        else:
            u = torch.einsum("ohf,bfd->bohd", w3, x)
            xv = torch.einsum("bohd,bhd->bod", u, xv) + b[None, :, None]
            outs.append(xv.sum(dim=2))
    return torch.cat(outs, dim=1)


def cin_literal(x, ws, bs, gy, dtype=torch.float64):
    """x [B, F, D], ws: L tensors [O_i, H_i F, 1], bs: L tensors [O_i], gy [B, sum O] -> {"y", "gx", "gw", "gb"} (lists)"""
    x, ws, bs = _leaves(x, ws, bs, dtype)
    return _finish(literal_forward(x, ws, bs), x, ws, bs, gy)


def cin_factored(x, ws, bs, gy, dtype=torch.float64):
    x, ws, bs = _leaves(x, ws, bs, dtype)
    return _finish(factored_forward(x, ws, bs), x, ws, bs, gy)


def rel_err(got, want64):
    """max |got - fp64| / max(1, |fp64|) over the tensors of one kind"""
    err = 0.0
    for a, e in zip(got, want64):
        a = a.detach().cpu().to(torch.float64).reshape(e.shape)
        if e.numel():
            err = max(err, float(((a - e).abs() / e.abs().clamp(min=1.0)).max()))
    return err


def form_gaps(x, ws, bs, gy, want64, stored=None):
    """per kind: the larger of the fp32 literal form's (or, given, the stored reference's) and the fp32 factored form's distance
    to the float64 evaluation of the same inputs"""
    lit = stored if stored is not None else {k: rel_err(v, want64[k]) for k, v in cin_literal(x, ws, bs, gy, torch.float32).items()}
    fac = cin_factored(x, ws, bs, gy, torch.float32)
    return {k: max(float(lit[k]), rel_err(fac[k], want64[k])) for k in KINDS}


def check(got, want64, gaps, what):
    """every kind within max(4 x gap, 2^-20); prints each figure before it asserts"""
    bad = []
    for k in KINDS:
        err, bound = rel_err(got[k], want64[k]), max(4.0 * gaps[k], FLOOR)
        print(f"{what} {k}: err {err:.3e} gap {gaps[k]:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, f"{what}: {bad}"


def draw(B, F, D, layers, seed):
    """x ~ 0.5 N(0,1), W and c uniform within 1/sqrt(H F) (Conv1d's default), gy ~ N(0,1)"""
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(B, F, D, generator=g)
    ws, bs, H = [], [], F
    for o in layers:
        bound = 1.0 / (H * F) ** 0.5
        ws.append((torch.rand(o, H * F, 1, generator=g) * 2 - 1) * bound)
        bs.append((torch.rand(o, generator=g) * 2 - 1) * bound)
        H = o
    gy = torch.randn(B, sum(layers), generator=g)
    return x, ws, bs, gy
