"""The fused losses of torcheasyrec_amd.losses (csrc/loss_ops.hip) against the reference's own modules
(tests/golden/reference_loss_vectors.npz: JRCLoss and BinaryFocalLoss run in fp32 and fp64) and against the float64 restatement
tests/loss_ref.py: on the lane emulator here, on the gfx950 library under `-m gpu`.

Bounds: the kernels sum in another order than torch, so the bound of a kind is 4 x the gap torch's (or the reference
module's) own fp32 result has to fp64 on these inputs, `ref_gap/<kind>` of the npz -- on |ours - fp64| / max(1, |fp64|) for
the loss, on |ours - fp64| of B * gradient for the gradient.  With the committed npz:

    kind                    loss       B * gradient
    binary_cross_entropy    5.8e-07    1.5e-06
    binary_focal_loss       3.8e-07    1.4e-06
    l2_loss                 5.0e-07    1.8e-04   (logits of scale 30: 2 (x - y) is of the order of 100)
    softmax_cross_entropy   1.1e-06    2.1e-06
    jrc_loss                4.4e-07    3.6e-06

Every figure is printed before it is asserted (pytest -s shows them).
"""
import os

import numpy as np
import pytest
import torch

import loss_ref as ref
from torcheasyrec_amd import losses as L

NPZ = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_loss_vectors.npz"))
_REF_CACHE = {}


def bounds(kind):
    return 4.0 * float(NPZ[f"ref_gap/{kind}/loss"]), 4.0 * float(NPZ[f"ref_gap/{kind}/grad"])


def run(dev, fn, logits):
    x = logits.detach().clone().to(dev).requires_grad_(True)
    loss = fn(x)
    loss.backward()
    return loss.detach().cpu().double(), x.grad.detach().cpu().double()


def check(kind, what, ours, want, B):
    (l, g), (wl, wg) = ours, want
    el = float((l - wl).abs() / max(1.0, float(wl.abs())))
    eg = float((g - wg).abs().max()) * B
    bl, bg = bounds(kind)
    print(f"{kind} {what}: loss err {el:.3e} (bound {bl:.3e})  B*grad err {eg:.3e} (bound {bg:.3e})")
    assert torch.isfinite(l) and el <= bl, (kind, what, el, bl)
    assert eg <= bg, (kind, what, eg, bg)


def cached(key, make):
    if key not in _REF_CACHE:
        _REF_CACHE[key] = make()
    return _REF_CACHE[key]


WEIGHT_MODES = ("none", "weights", "zeros", "space_1_0", "space_2_05_task_03")


def weight_mode(mode, B, dev):
    """(RowWeights for the kernel, keyword arguments for loss_ref.loss_and_grad)"""
    w, s = ref.weight_inputs(B)
    if mode == "none":
        return L.RowWeights(), {}
    if mode == "weights":
        return L.RowWeights(w.to(dev)), {"weight": w}
    if mode == "zeros":
        return L.RowWeights(torch.zeros(B, device=dev)), {"weight": torch.zeros(B)}
    if mode == "space_1_0":
        return L.RowWeights(None, s.to(dev), 1.0, 0.0), {"space_label": s, "in_w": 1.0, "out_w": 0.0}
    return (L.RowWeights(w.to(dev), s.to(torch.int32).to(dev), 2.0, 0.5, 0.3),
            {"weight": w, "space_label": s, "in_w": 2.0, "out_w": 0.5, "task_weight": 0.3})


# ---- the restatement is the reference's ---------------------------------------------------------------------------------
def test_restatement_reproduces_every_reference_case_in_fp64():
    for tag in NPZ["jrc/cases"]:
        x, y, sid, w = (torch.from_numpy(NPZ[f"{tag}/{k}"]) for k in ("logits", "labels", "session", "weight"))
        a = float(NPZ[f"{tag}/alpha"])
        for form, kw in (("mean", {}), ("weighted", {"weight": w})):
            l, g = ref.loss_and_grad("jrc_loss", x, y, sid, alpha=a, **kw)
            assert abs(float(l) - float(NPZ[f"{tag}/{form}/loss64"])) <= 1e-12, (tag, form)
            assert float((g - torch.from_numpy(NPZ[f"{tag}/{form}/grad64"])).abs().max()) <= 1e-12, (tag, form)
    assert round(float(NPZ["jrc/literal/mean/loss32"]), 4) == float(NPZ["jrc/literal/expected"]) == 0.7199
    for tag in NPZ["focal/cases"]:
        x, y, w = (torch.from_numpy(NPZ[f"{tag}/{k}"]) for k in ("logits", "labels", "weight"))
        for form, kw in (("mean", {}), ("weighted", {"weight": w})):
            l, g = ref.loss_and_grad("binary_focal_loss", x, y, gamma=float(NPZ[f"{tag}/gamma"]), alpha=float(NPZ[f"{tag}/alpha"]), **kw)
            assert abs(float(l) - float(NPZ[f"{tag}/{form}/loss64"])) <= 1e-12 * max(1.0, abs(float(l))), (tag, form)
            assert float((g - torch.from_numpy(NPZ[f"{tag}/{form}/grad64"])).abs().max()) <= 1e-12, (tag, form)


# ---- pointwise ----------------------------------------------------------------------------------------------------------
def _pointwise_cases():
    yield "binary_cross_entropy", L.LOSS_BCE, (0.0, 0.0), {"label_smoothing": 0.0}
    yield "binary_cross_entropy", L.LOSS_BCE, (0.1, 0.0), {"label_smoothing": 0.1}
    for gamma, alpha in ref.FOCAL_PARAMS:
        yield "binary_focal_loss", L.LOSS_FOCAL, (gamma, alpha), {"gamma": gamma, "alpha": alpha}
    yield "l2_loss", L.LOSS_L2, (0.0, 0.0), {}


@pytest.mark.parametrize("mode", WEIGHT_MODES)
@pytest.mark.parametrize("scale", ref.SCALES)
@pytest.mark.parametrize("B", ref.POINTWISE_B)
def test_pointwise_kinds(dev, B, scale, mode):
    x, y, t = ref.pointwise_inputs(B, scale)
    weights, kw = weight_mode(mode, B, dev)
    for i, (kind, code, (p0, p1), rkw) in enumerate(_pointwise_cases()):
        for dtype in (torch.float32, torch.int32, torch.int64):
            labels = t if (kind == "l2_loss" and dtype == torch.float32) else y.to(dtype)
            want = cached((kind, B, scale, mode, i, labels is t), lambda: ref.loss_and_grad(kind, x, labels, **rkw, **kw))
            fn = lambda v: L.pointwise_loss(code, v, labels.to(dev), p0, p1, weights)  # noqa: E731
            ours = run(dev, fn, x)
            if mode == "zeros":
                assert float(ours[0]) == 0.0 and not bool(ours[1].any())
            check(kind, f"B={B} x{scale} {mode} {dtype} {rkw}", ours, want, B)
            again = run(dev, fn, x)
            assert torch.equal(ours[0], again[0]) and torch.equal(ours[1], again[1])


def test_focal_against_the_reference_module(dev):
    for tag in NPZ["focal/cases"]:
        x, y, w = (torch.from_numpy(NPZ[f"{tag}/{k}"]) for k in ("logits", "labels", "weight"))
        g, a = float(NPZ[f"{tag}/gamma"]), float(NPZ[f"{tag}/alpha"])
        for form, weights in (("mean", L.RowWeights()), ("weighted", L.RowWeights(w.to(dev)))):
            ours = run(dev, lambda v: L.pointwise_loss(L.LOSS_FOCAL, v, y.to(dev), g, a, weights), x)
            want = torch.tensor(float(NPZ[f"{tag}/{form}/loss64"]), dtype=torch.float64), torch.from_numpy(NPZ[f"{tag}/{form}/grad64"])
            check("binary_focal_loss", f"{tag} {form}", ours, want, x.shape[0])


# ---- softmax cross entropy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("none", "space_2_05_task_03"))
@pytest.mark.parametrize("eps", (0.0, 0.1))
@pytest.mark.parametrize("C", ref.SOFTMAX_C)
@pytest.mark.parametrize("B", ref.SOFTMAX_B)
def test_softmax_cross_entropy(dev, B, C, eps, mode):
    x, y = ref.softmax_inputs(B, C)
    weights, kw = weight_mode(mode, B, dev)
    want = ref.loss_and_grad("softmax_cross_entropy", x, y, label_smoothing=eps, **kw)
    for dtype in (torch.int64, torch.int32):
        fn = lambda v: L.softmax_cross_entropy(v, y.to(dtype).to(dev), eps, weights)  # noqa: E731
        ours = run(dev, fn, x)
        check("softmax_cross_entropy", f"B={B} C={C} eps={eps} {mode} {dtype}", ours, want, B)
        again = run(dev, fn, x)
        assert torch.equal(ours[0], again[0]) and torch.equal(ours[1], again[1])
    # a row stride that is not C: the logits are the left columns of a wider tensor
    wide = torch.cat([x, torch.full((B, 3), 1e30)], dim=1).to(dev).requires_grad_(True)
    loss = L.softmax_cross_entropy(wide[:, :C], y.to(dev), eps, weights)
    loss.backward()
    strided = loss.detach().cpu().double(), wide.grad[:, :C].detach().cpu().double()
    assert torch.equal(strided[0], ours[0]) and torch.equal(strided[1], ours[1])
    assert not bool(wide.grad[:, C:].any())


@pytest.mark.parametrize("C", (3, 65))
def test_softmax_label_out_of_range_is_counted_not_indexed(dev, C):
    B = 257
    x, y = ref.softmax_inputs(B, C)
    bad = y.clone()
    bad[100] = C + 5
    counter = torch.zeros((), dtype=torch.int64, device=dev)
    good = run(dev, lambda v: L.softmax_cross_entropy(v, y.to(dev), 0.1, bad_labels=counter), x)
    assert int(counter) == 0
    ours = run(dev, lambda v: L.softmax_cross_entropy(v, bad.to(dev), 0.1, bad_labels=counter), x)
    assert int(counter) == 1
    assert not bool(ours[1][100].any())
    keep = torch.arange(B) != 100
    assert torch.equal(ours[1][keep], good[1][keep])
    # the row adds nothing to the sum, and still counts in the normaliser
    rows = ref.softmax_rows(x.double(), y, 0.1)
    want = (rows.sum() - rows[100]) / B
    assert abs(float(ours[0]) - float(want)) <= bounds("softmax_cross_entropy")[0] * max(1.0, float(want))
    bad[7] = -1
    run(dev, lambda v: L.softmax_cross_entropy(v, bad.to(dev), 0.1, bad_labels=counter), x)
    assert int(counter) == 3


# ---- JRC ---------------------------------------------------------------------------------------------------------------
def _jrc(dev, x, y, sid, alpha, weights=None):
    return lambda v: L.jrc_loss(v, y.to(dev), sid.to(dev), alpha, weights if weights is not None else L.RowWeights())


def test_jrc_against_the_reference_module(dev):
    for tag in NPZ["jrc/cases"]:
        x, y, sid, w = (torch.from_numpy(NPZ[f"{tag}/{k}"]) for k in ("logits", "labels", "session", "weight"))
        a = float(NPZ[f"{tag}/alpha"])
        for form, weights in (("mean", None), ("weighted", L.RowWeights(w.to(dev)))):
            ours = run(dev, _jrc(dev, x, y, sid, a, weights), x)
            want = torch.tensor(float(NPZ[f"{tag}/{form}/loss64"]), dtype=torch.float64), torch.from_numpy(NPZ[f"{tag}/{form}/grad64"])
            check("jrc_loss", f"{tag} {form}", ours, want, x.shape[0])
    x, y, sid = (torch.from_numpy(NPZ[f"jrc/literal/{k}"]) for k in ("logits", "labels", "session"))
    loss, _ = run(dev, _jrc(dev, x, y, sid, 0.5), x)
    assert round(float(loss), 4) == 0.7199


def _jrc_sessions(B, layout):
    x, y, sid = ref.jrc_inputs(B, max(B // 9, 1))
    if layout == "distinct":
        sid = torch.randperm(B, generator=torch.Generator().manual_seed(B)) * 3 - B
    elif layout == "one":
        sid = torch.full((B,), 42, dtype=torch.int64)
    elif layout == "wide_ids":  # negative ids and ids above 2^40, interleaved
        sid = torch.where(sid % 2 == 0, sid + (1 << 41), -sid - 5)
    return x, y, sid


@pytest.mark.parametrize("mode", ("none", "weights", "space_2_05_task_03"))
@pytest.mark.parametrize("alpha", (0.5, 0.2, 1.0))
@pytest.mark.parametrize("layout", ("interleaved", "distinct", "one", "wide_ids"))
@pytest.mark.parametrize("B", ref.JRC_B)
def test_jrc_shapes_and_sessions(dev, B, layout, alpha, mode):
    x, y, sid = _jrc_sessions(B, layout)
    weights, kw = weight_mode(mode, B, dev)
    want = cached(("jrc", B, layout, alpha, mode), lambda: ref.loss_and_grad("jrc_loss", x, y, sid, alpha=alpha, **kw))
    for dtype in (torch.int64, torch.float32):
        fn = _jrc(dev, x, y.to(dtype), sid, alpha, weights)
        ours = run(dev, fn, x)
        check("jrc_loss", f"B={B} {layout} alpha={alpha} {mode} {dtype}", ours, want, B)
    again = run(dev, fn, x)
    assert torch.equal(ours[0], again[0]) and torch.equal(ours[1], again[1])


def test_jrc_sessions_of_one_class_and_a_batch_of_negatives(dev):
    # session 5 has no positive row, session 6 no negative, session 7 both; the batch holds both classes
    sid = torch.tensor([7, 5, 6, 7, 5, 6, 7, 5, 6, 7, 7, 5])
    y = torch.tensor([1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0])
    x = ref.jrc_inputs(12, 3)[0]
    for alpha in (0.5, 0.2):
        check("jrc_loss", "one-class sessions", run(dev, _jrc(dev, x, y, sid, alpha), x), ref.loss_and_grad("jrc_loss", x, y, sid, alpha=alpha), 12)
    # only negatives: the reference's mean form is NaN here; the kernel returns the finite closed form
    x, _, sid = ref.jrc_inputs(300, 11)
    y = torch.zeros(300, dtype=torch.int64)
    want = ref.loss_and_grad("jrc_loss", x, y, sid, alpha=0.5)
    assert torch.isfinite(want[0])
    check("jrc_loss", "only negatives", run(dev, _jrc(dev, x, y, sid, 0.5), x), want, 300)
