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

That rule was measured on the npz's inputs.  The cases behind `check_literal` (batches past one tile per workgroup and past 256
workgroups, saturated, large and masked logits, placed JRC sessions) draw other scales and longer sums, so their bound is
max(the bound above, 4 x the distance of the fp32 literal form to float64 on the same inputs): `loss_ref.loss_and_grad_fp32`, the
same loss_ref.ROWS expression and weight combination on float32 tensors with autograd (the rule of tests/test_wukong_kernels.py).
Measured over those cases, ours / literal, smallest to largest, the same on the lane emulator and on the device but where noted:

    kind                    loss            B * gradient
    binary_cross_entropy    0.00 - 1.05     1.00 - 1.47
    binary_focal_loss       0.00 - 12.36    1.00 - 1.46
    l2_loss                 0.14 - 5.48     0.51 - 1.53   (device: 1.00 - 5.48, 0.89 - 1.53)
    softmax_cross_entropy   0.02 - 65.11    0.41 - 2.47   (device: gradient 0.50 - 2.47)
    jrc_loss                0.06 - 12.14    0.04 - 1.60   (device: 0.03 - 4.28, 0.03 - 0.93)

The loss ratios above 4 are cases whose literal form happens to land within 1e-8 of float64 (1.8e-9 for the 65.11, softmax x 40
at C = 40 with smoothing): there the npz bound decides, and the largest error / bound over all of these cases is 0.47 (focal loss)
and 0.27 (focal gradient), on both.  Before the row loss and the gradient were formed as (m - x) + log(s) instead of x - lse, the
softmax gradient at logits x 40 was 35 - 135 x the literal form's distance (B * gradient error 6.7e-6 - 1.5e-5, bound 2.1e-6).

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


# ---- past one tile, past 256 workgroups; saturated, large and masked logits; placed sessions -------------------------------
LS_THREADS, LS_ITEMS, LS_MAX_PARTS, LS_SMALL_C = 256, 4, 4096, 8  # csrc/loss_ops.hip
LS_TILE = LS_THREADS * LS_ITEMS
B_FINISH = 262144 + 1029  # more than LS_THREADS workgroups: tzr_loss_finish_kernel's loop over the partials runs twice
B_WALK = 4194304 + 5      # more than LS_MAX_PARTS tiles: a workgroup walks two tiles, and the last workgroup is partial


def ls_partition(B):
    """(workgroups, rows per workgroup): ls_partition of csrc/loss_ops.hip"""
    n_wg, per_wg = -(-B // LS_TILE), LS_TILE
    if n_wg > LS_MAX_PARTS:
        per_wg = -(-(-(-B // LS_MAX_PARTS)) // LS_TILE) * LS_TILE
        n_wg = -(-B // per_wg)
    return n_wg, per_wg


def test_the_big_batches_take_the_second_trip_of_both_loops():
    src = open(os.path.join(os.path.dirname(__file__), "..", "torcheasyrec_amd", "csrc", "loss_ops.hip")).read()
    for name, value in (("LS_THREADS", LS_THREADS), ("LS_ITEMS", LS_ITEMS), ("LS_MAX_PARTS", LS_MAX_PARTS), ("LS_SMALL_C", LS_SMALL_C)):
        assert f"#define {name} {value}" in src, name  # the constants restated above are the kernels'
    n_wg, per_wg = ls_partition(B_FINISH)
    assert per_wg == LS_TILE and LS_THREADS < n_wg <= 2 * LS_THREADS and B_FINISH % LS_TILE != 0
    assert -(-B_WALK // LS_TILE) > LS_MAX_PARTS
    n_wg, per_wg = ls_partition(B_WALK)
    assert per_wg == 2 * LS_TILE and n_wg > LS_THREADS and 0 < B_WALK - (n_wg - 1) * per_wg < LS_TILE
    assert max(ref.POINTWISE_B) <= LS_MAX_PARTS * LS_TILE and 2 <= LS_SMALL_C  # (C = 2 below is the lane-per-row kernel)


def check_literal(kind, what, ours, want, lit, B, dev):
    """`check` with the bound max(bounds(kind), 4 x the fp32 literal form's own distance to float64 on these inputs)"""
    (l, g), (wl, wg), (ll, lg) = ours, want, lit
    den = max(1.0, float(wl.abs()))
    el, gl = float((l - wl).abs()) / den, float((ll - wl).abs()) / den
    eg, gg = float((g - wg).abs().max()) * B, float((lg - wg).abs().max()) * B
    bl, bg = (max(b, 4.0 * gap) for b, gap in zip(bounds(kind), (gl, gg)))
    ratio = lambda e, gap: f"{e / gap:.2f}" if gap > 0 else "-"  # noqa: E731
    print(f"{kind} {what} on {dev.type}: loss err {el:.3e} literal {gl:.3e} bound {bl:.3e} ours/literal {ratio(el, gl)}"
          f"  B*grad err {eg:.3e} literal {gg:.3e} bound {bg:.3e} ours/literal {ratio(eg, gg)}")
    assert torch.isfinite(l) and bool(torch.isfinite(g).all()), (kind, what)
    assert el <= bl, (kind, what, el, bl)
    assert eg <= bg, (kind, what, eg, bg)


def _both_refs(key, kind, x, labels, *args, **kw):
    return cached(key, lambda: (ref.loss_and_grad(kind, x, labels, *args, **kw), ref.loss_and_grad_fp32(kind, x, labels, *args, **kw)))


def _twice(dev, fn, x):
    ours, again = run(dev, fn, x), run(dev, fn, x)
    assert torch.equal(ours[0], again[0]) and torch.equal(ours[1], again[1]), "two runs of the same case differ"
    return ours


def _big_cases():
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    for i, (kind, code, params, rkw) in enumerate(_pointwise_cases()):  # every pointwise kind through the finishing loop's second trip
        yield f"finish-{kind}-{i}", B_FINISH, kind, code, params, rkw, (1.0, 30.0)[i % 2], "space_2_05_task_03", (i64, i32, f32)[i % 3]
    yield "finish-softmax", B_FINISH, "softmax_cross_entropy", None, (0.0,), {"label_smoothing": 0.0}, 1.0, "space_2_05_task_03", i32
    yield "walk-bce", B_WALK, "binary_cross_entropy", L.LOSS_BCE, (0.0, 0.0), {"label_smoothing": 0.0}, 1.0, "none", i64
    yield "walk-focal", B_WALK, "binary_focal_loss", L.LOSS_FOCAL, (1.5, 0.75), {"gamma": 1.5, "alpha": 0.75}, 30.0, "weights", i32
    yield "walk-l2", B_WALK, "l2_loss", L.LOSS_L2, (0.0, 0.0), {}, 30.0, "space_2_05_task_03", f32
    yield "walk-softmax", B_WALK, "softmax_cross_entropy", None, (0.1,), {"label_smoothing": 0.1}, 1.0, "space_2_05_task_03", i64


_BIG = list(_big_cases())


@pytest.mark.parametrize("case", _BIG, ids=[c[0] for c in _BIG])
def test_batches_past_one_tile_per_workgroup_and_past_256_workgroups(dev, case):
    tag, B, kind, code, params, rkw, scale, mode, dtype = case
    weights, kw = weight_mode(mode, B, dev)
    if kind == "softmax_cross_entropy":  # C = 2: one lane per row; its row losses go through tzr_loss_rows_kernel, as JRC's do
        x, y = ref.softmax_inputs(B, 2)
        labels = y.to(dtype)
        fn = lambda v: L.softmax_cross_entropy(v, labels.to(dev), params[0], weights)  # noqa: E731
    else:
        x, y, t = ref.pointwise_inputs(B, scale)
        labels = t if (kind == "l2_loss" and dtype == torch.float32) else y.to(dtype)
        fn = lambda v: L.pointwise_loss(code, v, labels.to(dev), params[0], params[1], weights)  # noqa: E731
    want, lit = _both_refs(("big", tag), kind, x, labels, **rkw, **kw)
    check_literal(kind, f"{tag} B={B} x{scale} {mode} {dtype}", _twice(dev, fn, x), want, lit, B, dev)


def _saturated_cases():
    yield "binary_cross_entropy", L.LOSS_BCE, (0.0, 0.0), {"label_smoothing": 0.0}
    yield "binary_cross_entropy", L.LOSS_BCE, (0.1, 0.0), {"label_smoothing": 0.1}
    for gamma, alpha in ref.FOCAL_PARAMS:  # gamma 0 at p = 0 is pow(0, 0)
        yield "binary_focal_loss", L.LOSS_FOCAL, (gamma, alpha), {"gamma": gamma, "alpha": alpha}


@pytest.mark.parametrize("case", list(_saturated_cases()), ids=lambda c: f"{c[0]}-{c[2][0]}-{c[2][1]}")
def test_saturated_pointwise_logits(dev, case):
    kind, code, (p0, p1), rkw = case
    xs = torch.tensor(ref.SATURATED_X, dtype=torch.float32).repeat_interleave(2)
    ys = torch.tensor([0, 1], dtype=torch.int64).repeat(len(ref.SATURATED_X))
    assert float(torch.sigmoid(torch.tensor(-104.0))) == 0.0  # p = 0 in float32 is among them
    # each row alone (the loss is relative to its own size; 3e38 twice in one sum is past float32), then all but +-3e38 in one batch
    batches = [(xs[i:i + 1], ys[i:i + 1]) for i in range(xs.numel())] + [(xs[xs.abs() < 1e38], ys[xs.abs() < 1e38])]
    for x, y in batches:
        want, lit = ref.loss_and_grad(kind, x, y, **rkw), ref.loss_and_grad_fp32(kind, x, y, **rkw)
        assert torch.isfinite(want[0]) and bool(torch.isfinite(want[1]).all())
        ours = run(dev, lambda v: L.pointwise_loss(code, v, y.to(dev), p0, p1), x)
        what = f"x={x.item():g} y={y.item()}" if x.numel() == 1 else f"{x.numel()} saturated rows"
        check_literal(kind, f"{what} {rkw}", ours, want, lit, x.numel(), dev)


@pytest.mark.parametrize("eps", (0.0, 0.1))
@pytest.mark.parametrize("C", (5, 8, 9, 40, 130))
def test_softmax_logits_of_scale_120(dev, C, eps):
    """softmax_inputs x 40: |logit| up to about 400, exp overflows without the row's max"""
    B = 257
    x, y = ref.softmax_inputs(B, C)
    x = x * 40
    assert float(x.abs().max()) > 89.0  # (exp(89) is past float32)
    want, lit = (f("softmax_cross_entropy", x, y, label_smoothing=eps) for f in (ref.loss_and_grad, ref.loss_and_grad_fp32))
    ours = _twice(dev, lambda v: L.softmax_cross_entropy(v, y.to(dev), eps), x)
    check_literal("softmax_cross_entropy", f"x40 B={B} C={C} eps={eps}", ours, want, lit, B, dev)


@pytest.mark.parametrize("mode", ("none", "weights"))
@pytest.mark.parametrize("C", (3, 8, 9, 65))
def test_softmax_masked_classes(dev, C, mode):
    """classes masked out by -inf, never the label's.  label_smoothing 0: the loss is the finite lse - x_y (the smoothing term
    0 * (sum x = -inf) must not be formed) and a masked class's gradient is exactly 0.  label_smoothing 0.1: +inf, as torch's."""
    B = 33
    x, y, mask = ref.masked_softmax_inputs(B, C)
    assert bool(mask.any(1).all()) and not bool(mask[torch.arange(B), y].any()) and int((~mask[0]).sum()) == 1
    assert C <= 64 or bool(mask[:, 64:].any())  # the wave kernel: a masked class on a lane's second trip
    weights, kw = weight_mode(mode, B, dev)
    want, lit = (f("softmax_cross_entropy", x, y, label_smoothing=0.0, **kw) for f in (ref.loss_and_grad, ref.loss_and_grad_fp32))
    assert torch.isfinite(want[0]) and torch.isfinite(lit[0])
    fn = lambda v: L.softmax_cross_entropy(v, y.to(dev), 0.0, weights)  # noqa: E731
    ours = run(dev, fn, x)
    print(f"masked C={C} {mode} eps=0 on {dev.type}: loss {float(ours[0])!r}, float64 {float(want[0])!r}")
    check_literal("softmax_cross_entropy", f"masked B={B} C={C} eps=0 {mode}", ours, want, lit, B, dev)
    again = run(dev, fn, x)
    assert torch.equal(ours[0], again[0]) and torch.equal(ours[1], again[1])
    assert not bool(ours[1][mask].any()) and not bool(want[1][mask].any())
    # the row whose only unmasked class is its label: loss 0
    alone = run(dev, lambda v: L.softmax_cross_entropy(v, y[:1].to(dev), 0.0), x[:1])
    assert float(alone[0]) == 0.0 and not bool(alone[1].any())
    assert float(ref.loss_and_grad("softmax_cross_entropy", x[:1], y[:1])[0]) == 0.0
    # with smoothing a masked class costs +inf on both sides; the gradients stay finite
    want, lit = (f("softmax_cross_entropy", x, y, label_smoothing=0.1, **kw) for f in (ref.loss_and_grad, ref.loss_and_grad_fp32))
    ours = _twice(dev, lambda v: L.softmax_cross_entropy(v, y.to(dev), 0.1, weights), x)
    assert float(ours[0]) == float(want[0]) == float("inf")
    finite = torch.zeros((), dtype=torch.float64)
    check_literal("softmax_cross_entropy", f"masked B={B} C={C} eps=0.1 {mode} (gradient)", (finite, ours[1]), (finite, want[1]), (finite, lit[1]), B, dev)


@pytest.mark.parametrize("C", (3, 65))
def test_softmax_masked_class_next_to_a_label_out_of_range(dev, C):
    B = 33
    x, y, mask = ref.masked_softmax_inputs(B, C)
    bad = y.clone()
    bad[5] = C + 5
    counter = torch.zeros((), dtype=torch.int64, device=dev)
    ours = run(dev, lambda v: L.softmax_cross_entropy(v, bad.to(dev), 0.0, bad_labels=counter), x)
    assert int(counter) == 1 and not bool(ours[1][5].any()) and not bool(ours[1][mask].any())
    rows = ref.softmax_rows(x.double(), y, 0.0)
    want = (rows.sum() - rows[5]) / B  # the bad row adds nothing to the sum, and still counts in the normaliser
    rows32 = ref.softmax_rows(x, y, 0.0)
    gap = abs(float((rows32.sum() - rows32[5]) / B) - float(want)) / max(1.0, float(want))
    err = abs(float(ours[0]) - float(want)) / max(1.0, float(want))
    bound = max(bounds("softmax_cross_entropy")[0], 4.0 * gap)
    print(f"masked + bad label C={C} on {dev.type}: loss {float(ours[0])!r} err {err:.3e} literal {gap:.3e} bound {bound:.3e}")
    assert err <= bound
    good = run(dev, lambda v: L.softmax_cross_entropy(v, y.to(dev), 0.0), x)
    keep = torch.arange(B) != 5
    assert torch.equal(ours[1][keep], good[1][keep])


def test_the_placed_sessions_sit_where_the_jrc_kernel_branches():
    WAVE = 64
    sizes = list(ref.JRC_PLACED_SIZES)
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    ends = [s + n for s, n in zip(starts, sizes)]
    B = ends[-1]
    assert B == 1221
    assert any(s % WAVE == WAVE - 1 for s in starts) and sum(s % WAVE == 0 for s in starts) >= 2  # heads on lane 63 and lane 0
    assert any(e % WAVE == 0 and n > 1 for e, n in zip(ends, sizes))                                # a session ends on a wave boundary
    assert {(e - 1) // WAVE - s // WAVE + 1 for s, e in zip(starts, ends)} >= {1, 2, 3, 5}          # sessions over 1, 2, 3 and 5 waves
    assert any(s // LS_THREADS != (e - 1) // LS_THREADS for s, e in zip(starts, ends))              # and over a workgroup boundary
    # the last head of a wave finds its session's end by binary search over [wave end, B): inside the array, and at its end
    searched = [e for i, (s, e) in enumerate(zip(starts, ends)) if i + 1 == len(starts) or starts[i + 1] // WAVE != s // WAVE]
    assert any(e < B and e % WAVE != 0 for e in searched) and searched[-1] == B and sum(e == B for e in searched) == 1
    assert any(n == 1 for n in sizes)


@pytest.mark.parametrize("mode", ("weights", "space_2_05_task_03"))
@pytest.mark.parametrize("scale", (1.0, 8.0, 30.0))
@pytest.mark.parametrize("shuffled", (False, True), ids=("sorted", "shuffled"))
def test_jrc_placed_sessions_and_large_logits(dev, shuffled, scale, mode):
    x, y, sid = ref.jrc_placed_inputs(scale, shuffled)
    B = x.shape[0]
    assert bool((sid[1:] >= sid[:-1]).all()) != shuffled
    weights, kw = weight_mode(mode, B, dev)
    want, lit = _both_refs(("placed", shuffled, scale, mode), "jrc_loss", x, y, sid, alpha=0.3, **kw)
    ours = _twice(dev, _jrc(dev, x, y, sid, 0.3, weights), x)
    check_literal("jrc_loss", f"placed {'shuffled' if shuffled else 'sorted'} x{scale} {mode}", ours, want, lit, B, dev)


def test_jrc_session_of_weight_zero_and_one_class_neighbours(dev):
    # sessions in sorted order: 40 mixed rows of weight 0 | 65 positives | 65 negatives | 30 mixed rows
    sizes = (40, 65, 65, 30)
    x, y, sid = ref.jrc_placed_inputs(1.0, False, sizes)
    B = x.shape[0]
    y[40:105], y[105:170] = 1, 0
    w = ref.weight_inputs(B)[0]
    w[:40] = 0.0
    assert bool((y[:40] == 1).any()) and bool((y[:40] == 0).any()) and bool((y[170:] == 1).any()) and bool((y[170:] == 0).any())
    for alpha in (0.3, 1.0):
        want, lit = (f("jrc_loss", x, y, sid, alpha=alpha, weight=w) for f in (ref.loss_and_grad, ref.loss_and_grad_fp32))
        ours = _twice(dev, _jrc(dev, x, y, sid, alpha, L.RowWeights(w.to(dev))), x)
        check_literal("jrc_loss", f"zero-weight session, one-class neighbours alpha={alpha}", ours, want, lit, B, dev)
        assert not bool(ours[1][:40].any())  # rows of weight 0 get no gradient
