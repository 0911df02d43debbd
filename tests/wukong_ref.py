"""Restatement of a WuKong layer for the tests (tzrec/modules/interaction.py:236-378) in plain torch on the CPU in the dtype asked
for: the two per-sample operations of csrc/wukong.hip alone (`fm_literal`: X (X^T W) and the LayerNorm over the F k values;
`mix_literal`: lcb, the residual projection, the concat, the add and the LayerNorm over D) and the literal layer
(`layer_literal`, on the reference's state-dict keys), each written as the reference writes it -- permute, matmul, layer_norm,
concat, add -- with the gradients from autograd.  In float64 it is the truth the kernels are held to; in float32 it is the
yardstick (`gap`): the literal form's own distance to float64 on the same inputs.  Nothing here touches the package under test.
"""
import torch
import torch.nn.functional as F

from masknet_ref import EPS, FLOOR, KINK, check, rel_err  # noqa: F401  (the project's one bound and its one error measure)

FM_KINDS = ("out", "gx", "dW", "dgamma", "dbeta")
MIX_KINDS = ("out", "gx", "gfm", "dWl", "dWr", "dgamma", "dbeta")


def _prep(t, dtype):
    return t.detach().cpu().to(dtype).clone().requires_grad_(True)


def fm_literal(x, W, gamma, beta, gout, dtype=torch.float64, eps=EPS):
    """x [B, F, D], W [F, k], gamma / beta [F k], gout [B, F k] -> kind -> [tensor]"""
    x, W, gamma, beta = (_prep(t, dtype) for t in (x, W, gamma, beta))
    z = torch.matmul(x, torch.matmul(x.permute(0, 2, 1), W))
    out = F.layer_norm(z.reshape(x.shape[0], -1), (gamma.numel(),), gamma, beta, eps)
    out.backward(gout.detach().cpu().to(dtype))
    return {"out": [out.detach()], "gx": [x.grad], "dW": [W.grad], "dgamma": [gamma.grad], "dbeta": [beta.grad]}


def mix_literal(x, fm, Wl, Wr, gamma, beta, gout, dtype=torch.float64, eps=EPS):
    """x [B, F, D], fm [B, Ff, D], Wl [F, Fl], Wr [F, Ff + Fl] or None (the identity residual), gamma / beta [D],
    gout [B, Fo, D] -> kind -> [tensor] (dWr: empty without Wr)"""
    x, fm, Wl, gamma, beta = (_prep(t, dtype) for t in (x, fm, Wl, gamma, beta))
    Wr = None if Wr is None else _prep(Wr, dtype)
    lcb = (x.permute(0, 2, 1) @ Wl).permute(0, 2, 1)
    res = x if Wr is None else (x.permute(0, 2, 1) @ Wr).permute(0, 2, 1)
    out = F.layer_norm(torch.concat((fm, lcb), dim=1) + res, (gamma.numel(),), gamma, beta, eps)
    out.backward(gout.detach().cpu().to(dtype))
    return {"out": [out.detach()], "gx": [x.grad], "gfm": [fm.grad], "dWl": [Wl.grad], "dWr": [] if Wr is None else [Wr.grad],
            "dgamma": [gamma.grad], "dbeta": [beta.grad]}


def draw_fm(B, Fn, D, k, seed):
    """standard normal inputs (no LayerNorm row has a variance near zero), gamma ~ 1 + 0.3 N, beta ~ 0.3 N"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Fn, D, generator=g), torch.randn(Fn, k, generator=g), 1.0 + 0.3 * torch.randn(Fn * k, generator=g),
            0.3 * torch.randn(Fn * k, generator=g), torch.randn(B, Fn * k, generator=g))


def draw_mix(B, Fn, D, Fl, Ff, identity, seed):
    g = torch.Generator().manual_seed(seed)
    Fo = Ff + Fl
    assert not identity or Fn == Fo
    return (torch.randn(B, Fn, D, generator=g), torch.randn(B, Ff, D, generator=g), torch.randn(Fn, Fl, generator=g),
            None if identity else torch.randn(Fn, Fo, generator=g), 1.0 + 0.3 * torch.randn(D, generator=g),
            0.3 * torch.randn(D, generator=g), torch.randn(B, Fo, D, generator=g))


def layer_literal(x, sd, gy, dtype=torch.float64, eps=EPS):
    """WuKongLayer.forward on the parameters `sd` (the REFERENCE's state-dict keys: the FMB's MLP is
    `fmb.mlp.mlp.<i>.perceptron.0.{weight,bias}`, Linear -> ReLU per layer) -> {"y": [y], "gx": [gx], "g:<key>": [grad]},
    "kink": whether a ReLU pre-activation of the MLP lies within 2^-16 of zero"""
    x = _prep(x, dtype)
    p = {k: _prep(v, dtype) for k, v in sd.items()}
    B, Fn, D = x.shape
    z = torch.matmul(x, torch.matmul(x.permute(0, 2, 1), p["fmb.weight"]))
    h = F.layer_norm(z.reshape(B, -1), (p["fmb.norm.weight"].numel(),), p["fmb.norm.weight"], p["fmb.norm.bias"], eps)
    kink, i = False, 0
    while f"fmb.mlp.mlp.{i}.perceptron.0.weight" in p:
        a = F.linear(h, p[f"fmb.mlp.mlp.{i}.perceptron.0.weight"], p[f"fmb.mlp.mlp.{i}.perceptron.0.bias"])
        kink = kink or bool((a.detach().abs() < KINK).any())
        h, i = torch.relu(a), i + 1
    fm = F.linear(h, p["fmb.feature_out_liner.weight"], p["fmb.feature_out_liner.bias"]).view(B, -1, D)
    lcb = (x.permute(0, 2, 1) @ p["lcb.weight"]).permute(0, 2, 1)
    res = (x.permute(0, 2, 1) @ p["residual_projection.weight"]).permute(0, 2, 1) if "residual_projection.weight" in p else x
    y = F.layer_norm(torch.concat((fm, lcb), dim=1) + res, (D,), p["norm.weight"], p["norm.bias"], eps)
    y.backward(gy.detach().cpu().to(dtype))
    out = {"y": [y.detach()], "gx": [x.grad], "kink": kink}
    out.update({f"g:{k}": [v.grad] for k, v in p.items()})
    return out
