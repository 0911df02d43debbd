"""tzr_ln_mask_fwd / tzr_ln_mask_bwd (csrc/ln_mask.hip) called directly on tensors as they lie, against the float64 restatement of
the row op (tests/masknet_ref.py), in the three forms the module uses: shared x with masks and no ReLU (`LN(x) * m_j`),
per-output with ReLU and no mask (`relu(LN_j(z_j))` into a concat buffer), a single row with ReLU and one mask.

Bound, per tensor kind (out, gx, gm, ggamma, gbeta): |ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the distance of
torch's literal fp32 form on the CPU to float64 on the same inputs.  Rows holding a float64 ReLU pre-activation within 2^-16 of
zero are left out of the gradient comparisons (both sides run on the batch without them), at most 1 % of a case's rows.
Measured on the lane emulator over the cases below, the kernels' distance over the literal form's: out 0.43 - 1.15,
gx 0.42 - 1.09, gm 0.91 - 1.09, gbeta 0.49 - 1.91, ggamma 0.13 - 1.4 wherever the bound is above its floor ((5, 2, 1), whose
literal ggamma lands within 1e-8 by chance, is held by the floor 2^-20): the factor 4 suffices."""
import ctypes as C

import pytest
import torch

import masknet_ref as ref
from torcheasyrec_amd import _lib

# a launch holds at most 512 workgroups x 4 waves = 2048 samples at a time per grid slice (LM_MAXGRID, LM_WAVES of csrc/ln_mask.hip)
CONCURRENT = 512 * 4
SHAPES = [(5, 2, 1), (1, 64, 3), (33, 65, 2), (70, 1024, 8), (4 * CONCURRENT + 37, 33, 2)]
FORMS = {"shared_masks": (True, False, True), "per_output_relu": (False, True, False), "single_relu_mask": (False, True, True)}  # shared, relu, masked
PAD = 3  # columns on either side of the slices: they start 12 bytes behind a row's start; the row stride is no multiple of 4


def _wide(ts, dev, fill=float("nan")):
    """the [B, D] tensors `ts` as column slices of ONE wider tensor whose row stride is odd"""
    B, D = ts[0].shape
    width = len(ts) * D + 2 * PAD
    w = torch.full((B, width + (width % 4 == 0)), fill, dtype=torch.float32, device=dev)
    assert w.stride(0) % 4 != 0
    views = [w[:, PAD + j * D:PAD + (j + 1) * D] for j in range(len(ts))]
    for v, t in zip(views, ts):
        v.copy_(t)
    return w, views


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[_lib.ptr(t) for t in ts])


def _strides(ts):
    return (C.c_int64 * len(ts))(*[t.stride(0) for t in ts])


def _run_library(dev, xs, gammas, betas, ms, gouts, shared, relu, eps=ref.EPS, backward=True):
    lib, n_out, n_x = _lib.lib(), len(gouts), len(xs)
    B, D = xs[0].shape
    _, xv = _wide(xs, dev)
    _, gv = _wide(gouts, dev)
    mv = _wide(ms, dev)[1] if ms else []
    gam, bet = [t.to(dev) for t in gammas], [t.to(dev) for t in betas]
    outw, outv = _wide([torch.zeros(B, D)] * n_out, dev)
    gxw, gxv = _wide([torch.zeros(B, D)] * n_x, dev)
    gmw, gmv = _wide([torch.zeros(B, D)] * n_out, dev) if ms else (None, [])
    stats = torch.empty(B, n_x, 2, dtype=torch.float32, device=dev)
    dgb = torch.empty(2, n_x, D, dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    rc = lib.tzr_ln_mask_fwd(_ptrs(xv), _strides(xv), _ptrs(gam), _ptrs(bet), _ptrs(mv) if ms else None, _strides(mv) if ms else None,
                             _ptrs(outv), _strides(outv), n_out, int(shared), int(relu), eps, B, D, _lib.ptr(stats), st)
    assert rc == 0
    if not backward:
        return {"out": outv}
    ws = _lib.workspace(lib.tzr_ln_mask_bwd_workspace(B, D, n_out, int(shared)), dev)
    rc = lib.tzr_ln_mask_bwd(_ptrs(gv), _strides(gv), _ptrs(xv), _strides(xv), _ptrs(gam), _ptrs(bet), _ptrs(mv) if ms else None,
                             _strides(mv) if ms else None, _lib.ptr(stats), n_out, int(shared), int(relu), B, D, _ptrs(gxv), _strides(gxv),
                             _ptrs(gmv) if ms else None, _strides(gmv) if ms else None, _lib.ptr(dgb[0]), _lib.ptr(dgb[1]), _lib.ptr(ws),
                             ws.numel(), st)
    assert rc == 0
    # nothing outside the slices was written: the padding columns still hold the fill
    for w in (outw, gxw) + ((gmw,) if ms else ()):
        edge = torch.cat([w[:, :PAD], w[:, -PAD:]], dim=1)
        assert bool(torch.isnan(edge).all())
    return {"out": outv, "gx": gxv, "gm": gmv, "ggamma": [dgb[0, j] for j in range(n_x)], "gbeta": [dgb[1, j] for j in range(n_x)],
            "stats": [stats]}


def _bit_equal(a, b):
    return all(torch.equal(p, q) for k in a for p, q in zip(a[k], b[k]))


def _check_case(dev, B, D, n_out, form, seed, mean=0.0):
    shared, relu, masked = FORMS[form]
    if form == "single_relu_mask":
        n_out = 1
    ins = ref.draw_ln_mask(B, D, n_out, shared, relu, masked, seed, mean)
    what = f"{form} ({B}, {D}, {n_out}) mean {mean} on {dev.type}"
    want = ref.ln_mask_literal(*ins, shared, relu)
    lit = ref.ln_mask_literal(*ins, shared, relu, dtype=torch.float32)
    kink = bool(want["kink"].any())
    got = _run_library(dev, *ins, shared, relu, backward=not kink)
    ref.check(got, want, {"out": ref.rel_err(lit["out"], want["out"])}, what, ("out",))
    if kink:  # the gradients: every side on the batch without the rows at the kink
        xs, ms, gouts = ref.drop_rows(want["kink"], ins[0], ins[3], ins[4])
        ins = (xs, ins[1], ins[2], ms, gouts)
        want = ref.ln_mask_literal(*ins, shared, relu)
        assert not bool(want["kink"].any())
        lit = ref.ln_mask_literal(*ins, shared, relu, dtype=torch.float32)
        got = _run_library(dev, *ins, shared, relu)
        print(f"{what}: gradients over {xs[0].shape[0]} of {B} rows")
    kinds = ("gx", "gm", "ggamma", "gbeta")
    ref.check(got, want, {k: ref.rel_err(lit[k], want[k]) for k in kinds}, what, kinds)
    assert _bit_equal(got, _run_library(dev, *ins, shared, relu)), "two runs of the same case differ"
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("B,D,n_out", SHAPES)
def test_kernel_edges(dev, B, D, n_out, form):
    _check_case(dev, B, D, n_out, form, seed=B * 131 + D)


@pytest.mark.parametrize("form", list(FORMS))
def test_rows_with_mean_100_and_unit_spread(dev, form):
    """x = 100 + N(0, 1): E[x^2] - E[x]^2 in fp32 loses the variance's leading digits (10001 - 10000 at 2^-10 per unit);
    the second pass over (x - mean)^2 does not"""
    got = _check_case(dev, 40, 200, 2, form, seed=17, mean=100.0)
    mean, rstd = got["stats"][0][..., 0], got["stats"][0][..., 1]
    assert float((mean - 100.0).abs().max()) < 0.5 and 0.7 < float(rstd.min()) and float(rstd.max()) < 1.4


def test_a_one_pass_variance_would_miss_the_bound():
    """the case above separates the two: E[x^2] - E[x]^2 in fp32 on the same rows is outside 4 x gap"""
    xs, gammas, betas, _, gouts = ref.draw_ln_mask(40, 200, 1, True, False, False, seed=17, mean=100.0)
    want = ref.ln_mask_literal(xs, gammas, betas, [], gouts, True, False)
    lit = ref.ln_mask_literal(xs, gammas, betas, [], gouts, True, False, dtype=torch.float32)
    x = xs[0]
    m = x.mean(1, keepdim=True)
    var1 = (x * x).mean(1, keepdim=True) - m * m
    one_pass = (x - m) * torch.rsqrt(var1 + ref.EPS) * gammas[0] + betas[0]
    gap = ref.rel_err(lit["out"], want["out"])
    err = ref.rel_err([one_pass], want["out"])
    print(f"one-pass variance: err {err:.3e} gap {gap:.3e}")
    assert err > max(4.0 * gap, ref.FLOOR)
