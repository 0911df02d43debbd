"""tzr_wukong_fm_fwd / _bwd and tzr_wukong_mix_fwd / _bwd (csrc/wukong.hip) called directly on column slices of a wider tensor
with an odd row stride, against the float64 restatement of the two operations (tests/wukong_ref.py).

Bound, per tensor kind (fm: out, gx, dW, dgamma, dbeta; mix: out, gx, gfm, dWl, dWr, dgamma, dbeta):
|ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the distance of torch's literal fp32 form on the CPU to float64 on
the same inputs (the rule of tests/test_ln_mask_kernel.py).  Inputs are standard normal.
Measured on the lane emulator over the cases below, the kernels' distance over the literal form's (printed per case and kind):
fm out 0.66 - 1.50, gx 0.77 - 1.38, dW 0.42 - 0.97, dgamma 0.00 - 1.04, dbeta 0.23 - 1.21; mix out 0.35 - 1.57, gx 0.61 - 1.26,
gfm 0.74 - 1.32, dWl 0.24 - 0.88, dWr 0.45 - 1.26, dgamma 0.00 - 1.28, dbeta 0.12 - 2.67 (the 0.00: (1, 1, 1, 1, 1, 1), where the
kernels' dgamma is the float64 one); on the device the largest is fm dgamma 2.67 at B = 549:
the factor 4 suffices."""
import pytest
import torch

import wukong_ref as ref
from torcheasyrec_amd import _lib

WK_MAXGRID = 512  # csrc/wukong.hip: workgroups of a pass over the batch, forward and backward alike, one sample each at a time
# (B, F, D, k, Fl, Ff)
SHAPES = [(1, 1, 1, 1, 1, 1), (5, 3, 8, 2, 3, 4), (7, 7, 20, 3, 3, 4), (3, 17, 33, 5, 9, 8), (3, 64, 128, 64, 32, 32), (9, 27, 128, 24, 16, 16),
          (WK_MAXGRID + 37, 3, 8, 2, 3, 4)]
PAD = 3  # columns on either side of a slice: it starts 12 bytes behind a row's start; the row stride is no multiple of 4


def _wide(t, dev, fill=float("nan")):
    """the [B, ...] tensor `t`, flattened to [B, n], as a column slice of a wider tensor whose row stride is odd"""
    t = t.reshape(t.shape[0], -1)
    B, n = t.shape
    width = n + 2 * PAD
    w = torch.full((B, width + (width % 2 == 0)), fill, dtype=torch.float32, device=dev)
    assert w.stride(0) % 2 == 1
    v = w[:, PAD:PAD + n]
    v.copy_(t)
    return w, v


def _untouched(w, n):
    return bool(torch.isnan(w[:, :PAD]).all()) and bool(torch.isnan(w[:, PAD + n:]).all())


def run_fm(dev, x, W, gamma, beta, gout):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    B, Fn, D = x.shape
    k = W.shape[1]
    n = Fn * k
    W, gamma, beta = (t.to(dev).contiguous() for t in (W, gamma, beta))
    _, xv = _wide(x, dev)
    _, gv = _wide(gout, dev)
    ow, ov = _wide(torch.zeros(B, n), dev)
    gxw, gxv = _wide(torch.zeros(B, Fn * D), dev)
    stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
    dp = torch.full((3 * n,), float("nan"), dtype=torch.float32, device=dev)
    assert lib.tzr_wukong_fm_fwd(p(xv), xv.stride(0), p(W), p(gamma), p(beta), ref.EPS, B, Fn, D, k, p(ov), ov.stride(0), p(stats), st) == 0
    ws = _lib.workspace(lib.tzr_wukong_fm_bwd_workspace(B, Fn, D, k), dev)
    assert lib.tzr_wukong_fm_bwd(p(gv), gv.stride(0), p(xv), xv.stride(0), p(W), p(gamma), p(stats), B, Fn, D, k, p(gxv), gxv.stride(0), p(dp),
                                 p(ws), ws.numel(), st) == 0
    assert _untouched(ow, n) and _untouched(gxw, Fn * D)  # nothing outside the slices was written
    return {"out": [ov], "gx": [gxv.reshape(B, Fn, D)], "dW": [dp[:n].view(Fn, k)], "dgamma": [dp[n:2 * n]], "dbeta": [dp[2 * n:]], "stats": [stats]}


def run_mix(dev, x, fm, Wl, Wr, gamma, beta, gout):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    B, Fn, D = x.shape
    Ff, Fl = fm.shape[1], Wl.shape[1]
    Fo = Ff + Fl
    Wl, gamma, beta = (t.to(dev).contiguous() for t in (Wl, gamma, beta))
    Wr = None if Wr is None else Wr.to(dev).contiguous()
    _, xv = _wide(x, dev)
    _, fv = _wide(fm, dev)
    _, gv = _wide(gout, dev)
    ow, ov = _wide(torch.zeros(B, Fo * D), dev)
    gxw, gxv = _wide(torch.zeros(B, Fn * D), dev)
    gfw, gfv = _wide(torch.zeros(B, Ff * D), dev)
    stats = torch.empty(B, Fo, 2, dtype=torch.float32, device=dev)
    a, b = Fn * Fo, Fn * Fo + Fn * Fl
    dp = torch.full((b + 2 * D,), float("nan"), dtype=torch.float32, device=dev)
    assert lib.tzr_wukong_mix_fwd(p(xv), xv.stride(0), p(fv), fv.stride(0), p(Wl), p(Wr), p(gamma), p(beta), ref.EPS, B, Fn, D, Ff, Fl, p(ov),
                                  ov.stride(0), p(stats), st) == 0
    ws = _lib.workspace(lib.tzr_wukong_mix_bwd_workspace(B, Fn, D, Ff, Fl), dev)
    assert lib.tzr_wukong_mix_bwd(p(gv), gv.stride(0), p(xv), xv.stride(0), p(fv), fv.stride(0), p(Wl), p(Wr), p(gamma), p(stats), B, Fn, D, Ff, Fl,
                                  p(gxv), gxv.stride(0), p(gfv), gfv.stride(0), p(dp), p(ws), ws.numel(), st) == 0
    assert _untouched(ow, Fo * D) and _untouched(gxw, Fn * D) and _untouched(gfw, Ff * D)
    return {"out": [ov.reshape(B, Fo, D)], "gx": [gxv.reshape(B, Fn, D)], "gfm": [gfv.reshape(B, Ff, D)], "dWl": [dp[a:b].view(Fn, Fl)],
            "dWr": [] if Wr is None else [dp[:a].view(Fn, Fo)], "dgamma": [dp[b:b + D]], "dbeta": [dp[b + D:]], "stats": [stats]}


def _bit_equal(a, b):
    return all(torch.equal(p, q) for k in a for p, q in zip(a[k], b[k]))


def _ratios(got, want, gaps, what, kinds):
    for k in kinds:
        if gaps[k] > 0:
            print(f"{what} {k}: ours / literal {ref.rel_err(got[k], want[k]) / gaps[k]:.2f}")


@pytest.mark.parametrize("B,Fn,D,k,Fl,Ff", SHAPES)
def test_fm_kernels(dev, B, Fn, D, k, Fl, Ff):
    ins = ref.draw_fm(B, Fn, D, k, seed=B * 131 + Fn * 17 + D)
    what = f"fm ({B}, {Fn}, {D}, {k}) on {dev.type}"
    want, lit = ref.fm_literal(*ins), ref.fm_literal(*ins, dtype=torch.float32)
    got = run_fm(dev, *ins)
    gaps = {kd: ref.rel_err(lit[kd], want[kd]) for kd in ref.FM_KINDS}
    _ratios(got, want, gaps, what, ref.FM_KINDS)
    ref.check(got, want, gaps, what, ref.FM_KINDS)
    assert _bit_equal(got, run_fm(dev, *ins)), "two runs of the same case differ"


@pytest.mark.parametrize("B,Fn,D,k,Fl,Ff", SHAPES)
def test_mix_kernels(dev, B, Fn, D, k, Fl, Ff):
    identity = Fn == Ff + Fl
    ins = ref.draw_mix(B, Fn, D, Fl, Ff, identity, seed=B * 137 + Fn * 19 + D)
    what = f"mix ({B}, {Fn}, {D}, {Fl}, {Ff}){' identity' if identity else ''} on {dev.type}"
    want, lit = ref.mix_literal(*ins), ref.mix_literal(*ins, dtype=torch.float32)
    got = run_mix(dev, *ins)
    gaps = {kd: ref.rel_err(lit[kd], want[kd]) for kd in ref.MIX_KINDS}
    _ratios(got, want, gaps, what, ref.MIX_KINDS)
    ref.check(got, want, gaps, what, ref.MIX_KINDS)
    assert _bit_equal(got, run_mix(dev, *ins)), "two runs of the same case differ"


def test_the_shapes_take_both_residuals_and_both_size_classes():
    ident = [s for s in SHAPES if s[1] == s[4] + s[5]]
    assert (7, 7, 20, 3, 3, 4) in ident and (3, 64, 128, 64, 32, 32) in ident and len(ident) < len(SHAPES)
    assert any(max(s[1], s[3], s[4] + s[5]) > 32 for s in SHAPES) and any(max(s[1], s[3], s[4] + s[5]) <= 32 for s in SHAPES)
    assert SHAPES[-1][0] > WK_MAXGRID and SHAPES[-1][0] % WK_MAXGRID != 0
