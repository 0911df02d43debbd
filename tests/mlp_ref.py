"""Restatement of the small dense layer stacks for the tests (tzrec/modules/mlp.py:58-83 as tzrec/models/dlrm.py:101-135 builds
them; the loss of rank_model.py:233-240) in plain torch on the CPU in the dtype asked for: the three operations of
csrc/mlp_ops.hip / csrc/mlp_mfma.hip (`mlp2_fwd_literal`, `mlp2_bwd_literal`, `tail_literal`).  In float64 it is the truth the
kernels are held to; in float32 it is the yardstick (`gap`): the literal form's own distance to float64 on the same inputs.
Nothing here touches the package under test.

The ReLU masks.  tzr_mlp2_bwd takes `ha` and `hb` as inputs and tzr_mlp_tail takes `y1`: their masks (`> 0`) are restated on
those very tensors, so kernel and reference share them exactly and no sign flip of a pre-activation can separate them.  The mask
of y2 is internal to the tail: `settle_tail` redraws the y1 rows that leave a y2 pre-activation so near zero that fp32 could
take the other side (a condition on the inputs, checked by the reference alone; no element is ever left out of a comparison)."""
import torch
import torch.nn.functional as F

import masknet_ref
from masknet_ref import FLOOR  # noqa: F401  (the project's one bound)

FWD_KINDS = ("ha", "hb")
BWD_KINDS = ("dWb", "dbb", "dWa", "dba")
TAIL_KINDS = ("logits", "loss", "g1", "db1", "dW2", "db2", "dw3", "db3")
# |pre_j| >= MARGIN * (|b2_j| + sum_k |y1_k W2_jk|) for every sample and unit j: 4 x the a-priori bound of an fp32 dot product of
# H1 + 1 terms, (H1 + 1) 2^-24 sum |terms|, at H1 = 64 (65 x 4 x 2^-24 < 2^-16)
MARGIN = 2.0 ** -16
MAX_PASSES = 8
LABEL_KINDS = ("int64", "int32", "float01", "soft")


def rel_err(got, want64):
    """the project's one error measure, max |got - fp64| / max(1, |fp64|) over the tensors of one kind -- but NaN as soon as a
    tensor of `got` holds a non-finite value or has another element count: the outputs under test start out NaN-filled, and
    max() over a tensor with a NaN is a NaN that Python's max(0.0, nan) drops, so masknet_ref.rel_err alone reports 0 for it"""
    if len(got) != len(want64):
        return float("nan")
    for a, e in zip(got, want64):
        if a.numel() != e.numel() or not bool(torch.isfinite(a).all()):
            return float("nan")
    return masknet_ref.rel_err(got, want64)


def check(got, want64, gaps, what, kinds):
    """every kind within max(4 x gap, 2^-20), a NaN error failing like any other miss; prints each figure before it asserts"""
    bad = []
    for k in kinds:
        err, bound = rel_err(got[k], want64[k]), max(4.0 * gaps[k], FLOOR)
        print(f"{what} {k}: err {err:.3e} gap {gaps[k]:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, f"{what}: {bad}"


def _c(t, dtype):
    return None if t is None else t.detach().cpu().to(dtype)


def mlp2_fwd_literal(x, Wa, ba, Wb, bb, dtype=torch.float64):
    """x [B, K0], Wa [H1, K0], ba [H1] or None, Wb [H2, H1], bb [H2] or None -> kind -> [tensor]"""
    x, Wa, ba, Wb, bb = (_c(t, dtype) for t in (x, Wa, ba, Wb, bb))
    ha = torch.relu(F.linear(x, Wa, ba))
    return {"ha": [ha], "hb": [torch.relu(F.linear(ha, Wb, bb))]}


def mlp2_bwd_literal(dhb, hb, ha, x, Wb, dtype=torch.float64):
    """the four parameter gradients as a function of the GIVEN activations (inputs of tzr_mlp2_bwd) -> kind -> [tensor]"""
    dhb, hb, ha, x, Wb = (_c(t, dtype) for t in (dhb, hb, ha, x, Wb))
    gb = dhb * (hb > 0)
    ga = (gb @ Wb) * (ha > 0)
    return {"dWb": [gb.t() @ ha], "dbb": [gb.sum(0)], "dWa": [ga.t() @ x], "dba": [ga.sum(0)]}


def tail_literal(y1, labels, W2, b2, w3, b3, dtype=torch.float64):
    """y1 [B, H1] (a ReLU output), labels [B], W2 [H2, H1], b2 [H2] or None, w3 [H2], b3 [1] or None -> kind -> [tensor]"""
    y1, W2, b2, w3, b3 = (_c(t, dtype) for t in (y1, W2, b2, w3, b3))
    y = labels.detach().cpu().to(dtype)
    B = y1.shape[0]
    pre = F.linear(y1, W2, b2)
    y2 = torch.relu(pre)
    z = y2 @ w3.reshape(-1)
    if b3 is not None:
        z = z + b3.reshape(())
    loss = (z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean()
    dl = (torch.sigmoid(z) - y) / B
    g2 = dl[:, None] * w3.reshape(1, -1) * (pre > 0)
    g1 = (g2 @ W2) * (y1 > 0)
    return {"logits": [z], "loss": [loss.reshape(1)], "g1": [g1], "db1": [g1.sum(0)], "dW2": [g2.t() @ y1], "db2": [g2.sum(0)],
            "dw3": [(dl[:, None] * y2).sum(0)], "db3": [dl.sum().reshape(1)]}


def _uniform(g, bound, *shape):
    return (torch.rand(*shape, generator=g) * 2.0 - 1.0) * bound


def negative_zeros(t, every=5):
    """every `every`-th exact zero of `t` becomes -0.0, in place; -> how many"""
    flat = t.view(-1)
    idx = (flat == 0).nonzero().view(-1)[::every]
    flat[idx] = -0.0
    return int(idx.numel())


def draw_mlp2(B, K0, H1, H2, seed):
    """weights within nn.Linear's default bounds (+- 1 / sqrt(fan_in)), x and dhb ~ N(0, 1) -> x, Wa, ba, Wb, bb, dhb"""
    g = torch.Generator().manual_seed(seed)
    ka, kb = K0 ** -0.5, H1 ** -0.5
    Wa, ba, Wb, bb = _uniform(g, ka, H1, K0), _uniform(g, ka, H1), _uniform(g, kb, H2, H1), _uniform(g, kb, H2)
    return torch.randn(B, K0, generator=g), Wa, ba, Wb, bb, torch.randn(B, H2, generator=g)


def given_activations(x, Wa, ba, Wb, bb):
    """ha, hb for tzr_mlp2_bwd: the fp32 literal forward's (about half of the entries exactly zero), a few of the zeros -0.0"""
    f = mlp2_fwd_literal(x, Wa, ba, Wb, bb, dtype=torch.float32)
    ha, hb = f["ha"][0].clone(), f["hb"][0].clone()
    negative_zeros(ha)
    negative_zeros(hb)
    return ha, hb


def tail_margin_rows(y1, W2, b2):
    """bool [B]: the rows of y1 with a y2 pre-activation nearer to zero than MARGIN x the sum of its terms' magnitudes"""
    y, W = y1.double(), W2.double()
    b = torch.zeros(W.shape[0], dtype=torch.float64) if b2 is None else b2.double()
    pre = y @ W.t() + b
    mag = y.abs() @ W.abs().t() + b.abs()
    return (pre.abs() < MARGIN * mag).any(dim=1)


def settle_tail(y1, W2, b2, g):
    """redraws (y1 = relu(N(0, 1)), generator `g`) the rows of y1 that break the margin condition, in place; at most
    MAX_PASSES passes (an all-zero row keeps the condition: pre = b2 exactly on both sides); then sets a few zeros to -0.0"""
    for n in range(MAX_PASSES + 1):
        bad = tail_margin_rows(y1, W2, b2)
        if not bool(bad.any()):
            break
        assert n < MAX_PASSES, f"{int(bad.sum())} rows still break the margin condition after {MAX_PASSES} passes"
        y1[bad] = torch.relu(torch.randn(int(bad.sum()), y1.shape[1], generator=g))
    assert not bool(tail_margin_rows(y1, W2, b2).any())
    negative_zeros(y1)
    return y1


def draw_labels(B, kind, g):
    hit = torch.rand(B, generator=g) < 0.3
    if kind == "soft":
        return torch.where(hit, torch.tensor(0.75), torch.tensor(0.25))
    return hit.to({"int64": torch.int64, "int32": torch.int32, "float01": torch.float32}[kind])


def draw_tail(B, H1, H2, seed, labels="int64", bias2=True, w3_scale=1.0, b3_shift=0.0, zero_row=None):
    """weights within nn.Linear's default bounds, y1 = relu(N(0, 1)) settled (`settle_tail`) against b2 -- or against no bias
    when the case passes none (`bias2` False: b2 is still returned, for the other cases of the test to ignore) -> y1, labels,
    W2, b2, w3, b3.  `w3_scale` / `b3_shift` widen and move the logits; `zero_row`: that row of y1 is all zero."""
    g = torch.Generator().manual_seed(seed)
    k2, k3 = H1 ** -0.5, H2 ** -0.5
    W2, b2, w3, b3 = _uniform(g, k2, H2, H1), _uniform(g, k2, H2), _uniform(g, k3, H2) * w3_scale, _uniform(g, k3, 1) + b3_shift
    y1 = torch.relu(torch.randn(B, H1, generator=g))
    if zero_row is not None:
        y1[zero_row] = 0.0
    settle_tail(y1, W2, b2 if bias2 else None, g)
    return y1, draw_labels(B, labels, g), W2, b2, w3, b3
