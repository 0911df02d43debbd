"""Restatement of MaskNet for the tests (tzrec/modules/masknet.py:77-85, 142-161) in plain torch on the CPU in the dtype asked
for: the literal module (`masknet_literal`) and the row op alone (`ln_mask_literal`: LayerNorm, an optional ReLU, an optional
mask, for several outputs).  In float64 it is the truth the kernels are held to; in float32 it is the yardstick (`gap`): the
literal form's own distance to float64 on the same inputs.  Nothing here touches the package under test.

The ReLU kink: an element whose float64 pre-activation lies within 2^-16 of zero may take either side in fp32.  The rows that
hold one (`kink` in the results) are left out of the gradient comparisons -- a row gradient by dropping the row, a sum over the
batch by taking the sum over the other rows, which both sides do by being run on the batch without them (`drop_rows`)."""
import torch
import torch.nn.functional as F

FLOOR = 2.0 ** -20  # 8 ulp of 1.0: guards the degenerate cases whose gap can land near zero by chance
KINK = 2.0 ** -16
EPS = 1e-5  # nn.LayerNorm's default


def _prep(t, dtype, grad=True):
    return t.detach().cpu().to(dtype).clone().requires_grad_(grad)


def _near_zero_rows(pre):
    return (pre.detach().abs() < KINK).any(dim=1)


def ln_mask_literal(xs, gammas, betas, ms, gouts, shared, relu, dtype=torch.float64, eps=EPS):
    """out_j = act(LN(x_j)) [* m_j].  xs / gammas / betas: one entry when `shared`, else one per output; ms: one per output or
    empty; gouts: one per output.  -> {"out", "gx", "gm", "ggamma", "gbeta"} as lists, "kink": bool [B]"""
    n_out = len(gouts)
    xs, gammas, betas, ms = ([_prep(t, dtype) for t in ts] for ts in (xs, gammas, betas, ms))
    kink = torch.zeros(xs[0].shape[0], dtype=torch.bool)
    outs = []
    for j in range(n_out):
        i = 0 if shared else j
        f = F.layer_norm(xs[i], xs[i].shape[1:], gammas[i], betas[i], eps)
        if relu:
            kink |= _near_zero_rows(f)
            f = torch.relu(f)
        outs.append(f * ms[j] if ms else f)
    torch.autograd.backward(outs, [g.detach().cpu().to(dtype) for g in gouts])
    return {"out": [o.detach() for o in outs], "gx": [x.grad for x in xs], "gm": [m.grad for m in ms],
            "ggamma": [g.grad for g in gammas], "gbeta": [b.grad for b in betas], "kink": kink}


LN_KINDS = ("out", "gx", "gm", "ggamma", "gbeta")


def masknet_literal(x, sd, n, parallel, gy, dtype=torch.float64, eps=EPS):
    """the module without its top MLP on the parameters `sd` (state-dict keys of MaskNetModule) -> {"y": [y], "gx": [gx],
    "g:<key>": [grad]} per parameter, "kink": bool [B]"""
    x = _prep(x, dtype)
    p = {k: _prep(v, dtype) for k, v in sd.items()}
    kink = torch.zeros(x.shape[0], dtype=torch.bool)

    def block(i, feat):
        nonlocal kink
        b = f"mask_blocks.{i}."
        a = F.linear(x, p[b + "mask_generator.0.weight"], p[b + "mask_generator.0.bias"])
        kink |= _near_zero_rows(a)
        m = F.linear(torch.relu(a), p[b + "mask_generator.2.weight"], p[b + "mask_generator.2.bias"])
        z = F.linear(feat * m, p[b + "ffn.0.weight"], p[b + "ffn.0.bias"])
        h = F.layer_norm(z, z.shape[1:], p[b + "ffn.1.weight"], p[b + "ffn.1.bias"], eps)
        kink |= _near_zero_rows(h)
        return torch.relu(h)

    ln = F.layer_norm(x, x.shape[1:], p["ln_emb.weight"], p["ln_emb.bias"], eps)
    if parallel:
        y = torch.cat([block(i, ln) for i in range(n)], dim=-1)
    else:
        y = block(0, ln)
        for i in range(1, n):
            y = block(i, y)
    y.backward(gy.detach().cpu().to(dtype))
    out = {"y": [y.detach()], "gx": [x.grad], "kink": kink}
    out.update({f"g:{k}": [v.grad] for k, v in p.items()})
    return out


def rel_err(got, want64, keep=None):
    """max |got - fp64| / max(1, |fp64|) over the tensors of one kind (over the rows `keep` of [B, .] tensors)"""
    err = 0.0
    for a, e in zip(got, want64):
        a = a.detach().cpu().to(torch.float64).reshape(e.shape)
        if keep is not None:
            a, e = a[keep], e[keep]
        if e.numel():
            err = max(err, float(((a - e).abs() / e.abs().clamp(min=1.0)).max()))
    return err


def check(got, want64, gaps, what, kinds):
    """every kind within max(4 x gap, 2^-20); prints each figure before it asserts"""
    bad = []
    for k in kinds:
        err, bound = rel_err(got[k], want64[k]), max(4.0 * gaps[k], FLOOR)
        print(f"{what} {k}: err {err:.3e} gap {gaps[k]:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, f"{what}: {bad}"


def drop_rows(kink, *tensor_lists):
    """the tensor lists without the rows marked in `kink`; at most 1 % of the rows may go"""
    n = int(kink.sum())
    assert n <= 0.01 * kink.numel(), f"{n} of {kink.numel()} rows hold a pre-activation within 2^-16 of zero"
    keep = ~kink
    return [[t[keep.to(t.device)] for t in ts] for ts in tensor_lists]


def draw_ln_mask(B, D, n_out, shared, relu, masked, seed, mean=0.0):
    """x ~ mean + N(0, 1), gamma ~ 1 + 0.3 N, beta ~ 0.3 N, m ~ N, gout ~ N.  Where fewer than 100 rows leave no room for the
    1 % of kink rows, an element whose float64 pre-activation is within 2^-12 of zero gets its x moved by 1/64 until none is."""
    g = torch.Generator().manual_seed(seed)
    n_x = 1 if shared else n_out
    xs = [mean + torch.randn(B, D, generator=g) for _ in range(n_x)]
    gammas = [1.0 + 0.3 * torch.randn(D, generator=g) for _ in range(n_x)]
    betas = [0.3 * torch.randn(D, generator=g) for _ in range(n_x)]
    ms = [torch.randn(B, D, generator=g) for _ in range(n_out)] if masked else []
    gouts = [torch.randn(B, D, generator=g) for _ in range(n_out)]
    if relu and B < 100 and D > 1:
        for i in range(n_x):
            for _ in range(20):
                f = F.layer_norm(xs[i].double(), (D,), gammas[i].double(), betas[i].double(), EPS)
                near = f.abs() < 2.0 ** -12
                if not bool(near.any()):
                    break
                xs[i] = torch.where(near, xs[i] + 1.0 / 64, xs[i])
    return xs, gammas, betas, ms, gouts
