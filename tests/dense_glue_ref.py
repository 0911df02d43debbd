"""Restatement of the small row-streaming operations of csrc/dense_ops.hip, csrc/gate_mix.hip and csrc/linear_bwd.hip for the
tests, in plain torch on the CPU in the dtype asked for.  Each operation is one `*_literal(inputs, dtype)`: in float64 it is the
truth the kernels are held to; in float32 it is the yardstick (`gap`): the literal form's own distance to float64 on the same
inputs.  Nothing here touches the package under test.

Every ReLU mask (`> 0`) is taken from a tensor the kernel also receives (`y` of relu_bwd_colsum and linear_bwd_relu, `x` of
head_bwd_relu), so kernel and reference share it exactly and no element is ever left out of a comparison.  The draws are
standard normal and unscaled: a sum over B rows is of the order of sqrt(B), and the error measure is a relative one."""
import torch
import torch.nn.functional as F

from mlp_ref import FLOOR, check, negative_zeros, rel_err  # noqa: F401  (the project's one bound; rel_err is NaN for an output that holds one)

RELU_KINDS = ("colsum",)
HEAD_KINDS = ("gw", "gb")
HEAD_RELU_KINDS = ("gw", "gb", "colsum")
SKINNY_KINDS = ("y", "gx", "gw", "gb")
MOE_KINDS = ("out", "probs", "d_logits", "d_expert")
LINEAR_BWD_KINDS = ("g", "colsum")
BCE_KINDS = ("loss", "grad")


def _c(t, dtype):
    return None if t is None else t.detach().cpu().to(dtype)


def relu_bwd_colsum_literal(gy, y, dtype=torch.float64):
    """gy, y [B, N] -> g = gy * (y > 0) and its column sums"""
    gy, y = _c(gy, dtype), _c(y, dtype)
    g = gy * (y > 0)
    return {"g": [g], "colsum": [g.sum(0)]}


def head_bwd_literal(gy, x, w, dtype=torch.float64):
    """backward of Linear(N, 1): gy [B], x [B, N], w [N] -> gx [B, N], gw [N], gb [1]"""
    gy, x, w = _c(gy, dtype).reshape(-1, 1), _c(x, dtype), _c(w, dtype).reshape(1, -1)
    return {"gx": [gy @ w], "gw": [(gy.t() @ x).reshape(-1)], "gb": [gy.sum(0)]}


def head_bwd_relu_literal(gy, x, w, dtype=torch.float64):
    """the same layer behind a ReLU whose output is x: g = (gy w) * (x > 0) [B, N], gw [N], gb [1], column sums of g [N]"""
    gy, x, w = _c(gy, dtype).reshape(-1, 1), _c(x, dtype), _c(w, dtype).reshape(1, -1)
    g = (gy @ w) * (x > 0)
    return {"g": [g], "gw": [(gy.t() @ x).reshape(-1)], "gb": [gy.sum(0)], "colsum": [g.sum(0)]}


def skinny_linear_literal(x, w, b, gy, dtype=torch.float64):
    """x [B, K], w [n, K], b [n] or None, gy [B, n] -> y = F.linear(x, w, b) and its three gradients under gy"""
    x, w, b, gy = (_c(t, dtype) for t in (x, w, b, gy))
    return {"y": [F.linear(x, w, b)], "gx": [gy @ w], "gw": [gy.t() @ x], "gb": [gy.sum(0)]}


def moe_mix_literal(experts, logits, gouts, dtype=torch.float64):
    """E experts [B, H], T gate logits [B, E], T upstream gradients [B, H]: stack, softmax, batched matmul and their autograd
    -> out [T], probs [T], d_logits [T], d_expert [E]"""
    xs = [_c(x, dtype).requires_grad_(True) for x in experts]
    ls = [_c(l, dtype).requires_grad_(True) for l in logits]
    st = torch.stack(xs, dim=1)
    probs = [torch.softmax(l, dim=1) for l in ls]
    outs = [torch.matmul(p.unsqueeze(1), st).squeeze(1) for p in probs]
    torch.autograd.backward(outs, [_c(g, dtype) for g in gouts])
    return {"out": [o.detach() for o in outs], "probs": [p.detach() for p in probs], "d_logits": [l.grad for l in ls],
            "d_expert": [x.grad for x in xs]}


def linear_bwd_relu_literal(gin, W, y, dtype=torch.float64):
    """gin [N, K], W [K, H], y [N, H] -> g = (gin W) * (y > 0) and its column sums"""
    gin, W, y = _c(gin, dtype), _c(W, dtype), _c(y, dtype)
    g = (gin @ W) * (y > 0)
    return {"g": [g], "colsum": [g.sum(0)]}


def bce_logits_literal(x, labels, sample_weight, dtype=torch.float64):
    """BCEWithLogitsLoss(reduction="mean"), with weights mean(loss_i w_i) -> loss [1] and B x d(loss)/d(logits) [B]"""
    x = _c(x, dtype).requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(x, _c(labels, dtype), weight=_c(sample_weight, dtype))
    loss.backward()
    return {"loss": [loss.detach().reshape(1)], "grad": [x.grad * x.numel()]}


def gaps(lit, want, kinds):
    return {k: rel_err(lit[k], want[k]) for k in kinds}


def relu_output(B, N, g):
    """relu(N(0, 1)) -- about half of the entries exactly zero -- with a few of the zeros -0.0 (which is not > 0 either)"""
    t = torch.relu(torch.randn(B, N, generator=g))
    negative_zeros(t)
    return t


def draw_relu(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, generator=g), relu_output(B, N, g)


def draw_head(B, N, seed, relu=False):
    """-> gy [B], x [B, N] (a ReLU output if `relu`), w [N]"""
    g = torch.Generator().manual_seed(seed)
    gy, w = torch.randn(B, generator=g), torch.randn(N, generator=g)
    return gy, (relu_output(B, N, g) if relu else torch.randn(B, N, generator=g)), w


def draw_skinny(B, K, n, seed):
    """-> x [B, K], w [n, K], b [n], gy [B, n]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, K, generator=g), torch.randn(n, K, generator=g), torch.randn(n, generator=g), torch.randn(B, n, generator=g)


def draw_moe(B, H, E, T, seed):
    """-> experts, logits, gouts.  Where B > 10 and E > 1, rows 0, 1, 2 of task 0's logits hold one logit at +80, all logits at
    -90, one logit at 1e4: fp32 exp() of the raw values is inf or 0 there, the float64 softmax is finite"""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, H, generator=g) for _ in range(E)]
    ls = [torch.randn(B, E, generator=g) for _ in range(T)]
    gos = [torch.randn(B, H, generator=g) for _ in range(T)]
    if B > 10 and E > 1:
        ls[0][0, E - 1] = 80.0
        ls[0][1, :] = -90.0
        ls[0][2, 0] = 1.0e4
    return xs, ls, gos


def draw_linear_bwd(N, K, H, seed):
    """-> gin [N, K], W [K, H], y [N, H] (a ReLU output)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, K, generator=g), torch.randn(K, H, generator=g), relu_output(N, H, g)


def draw_bce(B, label_kind, weighted, seed):
    """logits of scale 6 (saturated ones included, +-40 at the two ends), labels 0 / 1 in the dtype named, weights in [0.5, 1.5)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, generator=g) * 6.0
    x[0], x[-1] = 40.0, -40.0
    y = (torch.rand(B, generator=g) < 0.3).to({"float32": torch.float32, "int32": torch.int32, "int64": torch.int64}[label_kind])
    return x, y, (torch.rand(B, generator=g) + 0.5 if weighted else None)
