"""Error behaviour of the entry points of csrc/wukong.hip, as tests/test_masknet_abi.py checks their siblings: bad arguments come
back as negative status codes -- never a crash, never a launch -- and B == 0 is a TZR_OK no-op that writes nothing."""
import os

import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
B, F, D, K, FF, FL = 3, 5, 10, 3, 4, 3
FO = FF + FL
PADW = 2  # every per-sample stride below is the row's width + PADW


def _t(dev, *shape):
    return torch.ones(*shape, dtype=torch.float32, device=dev)


def _snapshot(dev, written):
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return [t.clone() for t in written]


def test_fm_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    x, gx = _t(dev, B, F * D + PADW), _t(dev, B, F * D + PADW)
    out, gout = _t(dev, B, F * K + PADW), _t(dev, B, F * K + PADW)
    w, gamma, beta = _t(dev, F, K), _t(dev, F * K) * 1.5, _t(dev, F * K) * 0.2
    stats, dp = _t(dev, B, 2), _t(dev, 3 * F * K)
    need = lib.tzr_wukong_fm_bwd_workspace(B, F, D, K)
    ws = _lib.workspace(need, dev)
    assert need == B * 3 * F * K * 4 + 256  # one row [dW | dgamma | dbeta] per workgroup, one workgroup per sample here (+ slack)

    def fwd(x_=p(x), xs=F * D + PADW, w_=p(w), g_=p(gamma), b_=p(beta), nb=B, f=F, d=D, k=K, o_=p(out), os_=F * K + PADW, st_=p(stats)):
        return lib.tzr_wukong_fm_fwd(x_, xs, w_, g_, b_, 1e-5, nb, f, d, k, o_, os_, st_, None)

    def bwd(go_=p(gout), gs=F * K + PADW, x_=p(x), xs=F * D + PADW, w_=p(w), g_=p(gamma), st_=p(stats), nb=B, f=F, d=D, k=K, gx_=p(gx),
            gxs=F * D + PADW, dp_=p(dp), ws_=p(ws), wsn=ws.numel()):
        return lib.tzr_wukong_fm_bwd(go_, gs, x_, xs, w_, g_, st_, nb, f, d, k, gx_, gxs, dp_, ws_, wsn, None)

    assert fwd() == OK and bwd() == OK
    assert fwd(xs=F * D, os_=F * K) == OK and bwd(gs=F * K, xs=F * D, gxs=F * D) == OK
    written = [out, gx, stats, dp]
    for t in written:
        t.fill_(7.0)
    before = _snapshot(dev, written)
    for fn, names in ((fwd, ("x_", "w_", "g_", "b_", "o_", "st_")), (bwd, ("go_", "x_", "w_", "g_", "st_", "gx_", "dp_"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name  # null pointer
        assert fn(nb=-1) == INVALID and fn(f=0) == INVALID and fn(d=0) == INVALID and fn(k=0) == INVALID and fn(d=-3) == INVALID
        assert fn(f=65) == UNSUPPORTED and fn(k=65) == UNSUPPORTED and fn(d=129) == UNSUPPORTED and fn(nb=1 << 30) == UNSUPPORTED  # one per limit
        assert fn(xs=F * D - 1) == UNSUPPORTED  # a short stride
        assert fn(f=0, d=129) == INVALID  # (the order: a size <= 0 before a limit)
    assert fwd(os_=F * K - 1) == UNSUPPORTED and bwd(gs=F * K - 1) == UNSUPPORTED and bwd(gxs=F * D - 1) == UNSUPPORTED
    assert bwd(ws_=None) == WORKSPACE and bwd(ws_=p(ws) + 4) == WORKSPACE  # no workspace, a misaligned one
    assert bwd(wsn=need - 256 - 1) == WORKSPACE and bwd(wsn=0) == WORKSPACE  # one byte short
    assert bwd(gs=F * K - 1, ws_=None) == UNSUPPORTED and bwd(x_=None, ws_=None) == INVALID  # (the order: the workspace comes last)
    # no sample: nothing is launched, nothing is read or written
    assert fwd(nb=0) == OK and bwd(nb=0) == OK
    assert fwd(nb=0, x_=None, w_=None, g_=None, b_=None, o_=None, st_=None) == OK
    assert bwd(nb=0, go_=None, x_=None, w_=None, g_=None, st_=None, gx_=None, dp_=None, ws_=None, wsn=0) == OK
    for a, b in zip(before, _snapshot(dev, written)):
        assert torch.equal(a, b)
    assert bwd(wsn=need - 256) == OK  # (the query's 256 bytes are the room to align in)


def test_mix_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    x, gx = _t(dev, B, F * D + PADW), _t(dev, B, F * D + PADW)
    fm, gfm = _t(dev, B, FF * D + PADW), _t(dev, B, FF * D + PADW)
    out, gout = _t(dev, B, FO * D + PADW), _t(dev, B, FO * D + PADW)
    wl, wr, gamma, beta = _t(dev, F, FL), _t(dev, F, FO), _t(dev, D) * 1.5, _t(dev, D) * 0.2
    stats, dp = _t(dev, B, FO, 2), _t(dev, F * FO + F * FL + 2 * D)
    need = lib.tzr_wukong_mix_bwd_workspace(B, F, D, FF, FL)
    ws = _lib.workspace(need, dev)
    assert need == B * (F * FO + F * FL + 2 * D) * 4 + 256  # one row [dWr | dWl | dgamma | dbeta] per workgroup (+ slack)

    def fwd(x_=p(x), xs=F * D + PADW, fm_=p(fm), fms=FF * D + PADW, wl_=p(wl), wr_=p(wr), g_=p(gamma), b_=p(beta), nb=B, f=F, d=D, ff=FF, fl=FL,
            o_=p(out), os_=FO * D + PADW, st_=p(stats)):
        return lib.tzr_wukong_mix_fwd(x_, xs, fm_, fms, wl_, wr_, g_, b_, 1e-5, nb, f, d, ff, fl, o_, os_, st_, None)

    def bwd(go_=p(gout), gs=FO * D + PADW, x_=p(x), xs=F * D + PADW, fm_=p(fm), fms=FF * D + PADW, wl_=p(wl), wr_=p(wr), g_=p(gamma), st_=p(stats),
            nb=B, f=F, d=D, ff=FF, fl=FL, gx_=p(gx), gxs=F * D + PADW, gf_=p(gfm), gfs=FF * D + PADW, dp_=p(dp), ws_=p(ws), wsn=ws.numel()):
        return lib.tzr_wukong_mix_bwd(go_, gs, x_, xs, fm_, fms, wl_, wr_, g_, st_, nb, f, d, ff, fl, gx_, gxs, gf_, gfs, dp_, ws_, wsn, None)

    assert fwd() == OK and bwd() == OK
    assert fwd(xs=F * D, fms=FF * D, os_=FO * D) == OK and bwd(gs=FO * D, xs=F * D, fms=FF * D, gxs=F * D, gfs=FF * D) == OK
    # the identity residual: no Wr, F == Fo (5 = 2 + 3; the tensors above are wide enough)
    assert fwd(wr_=None, ff=2) == OK and bwd(wr_=None, ff=2) == OK
    written = [out, gx, gfm, stats, dp]
    for t in written:
        t.fill_(7.0)
    before = _snapshot(dev, written)
    for fn, names in ((fwd, ("x_", "fm_", "wl_", "g_", "b_", "o_", "st_")), (bwd, ("go_", "x_", "fm_", "wl_", "g_", "st_", "gx_", "gf_", "dp_"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name  # null pointer
        assert fn(nb=-1) == INVALID and fn(f=0) == INVALID and fn(d=0) == INVALID and fn(ff=0) == INVALID and fn(fl=0) == INVALID and fn(fl=-2) == INVALID
        assert fn(f=65) == UNSUPPORTED and fn(d=129) == UNSUPPORTED and fn(nb=1 << 30) == UNSUPPORTED  # one per limit
        assert fn(ff=62) == UNSUPPORTED and fn(fl=61) == UNSUPPORTED and fn(ff=65) == UNSUPPORTED  # Fo = 65, 65, 68
        assert fn(wr_=None) == UNSUPPORTED  # a null Wr with F = 5 != Fo = 7
        assert fn(xs=F * D - 1) == UNSUPPORTED and fn(fms=FF * D - 1) == UNSUPPORTED  # short strides
        assert fn(fl=0, d=129) == INVALID
    assert fwd(os_=FO * D - 1) == UNSUPPORTED and bwd(gs=FO * D - 1) == UNSUPPORTED
    assert bwd(gxs=F * D - 1) == UNSUPPORTED and bwd(gfs=FF * D - 1) == UNSUPPORTED
    assert bwd(ws_=None) == WORKSPACE and bwd(ws_=p(ws) + 4) == WORKSPACE
    assert bwd(wsn=need - 256 - 1) == WORKSPACE and bwd(wsn=0) == WORKSPACE
    assert bwd(wr_=None, ws_=None) == UNSUPPORTED and bwd(x_=None, ws_=None) == INVALID
    assert fwd(nb=0) == OK and bwd(nb=0) == OK
    assert fwd(nb=0, x_=None, fm_=None, wl_=None, g_=None, b_=None, o_=None, st_=None) == OK
    assert bwd(nb=0, go_=None, x_=None, fm_=None, wl_=None, g_=None, st_=None, gx_=None, gf_=None, dp_=None, ws_=None, wsn=0) == OK
    for a, b in zip(before, _snapshot(dev, written)):
        assert torch.equal(a, b)
    assert bwd(wsn=need - 256) == OK


def test_workspace_queries_are_monotone_in_the_batch(dev):
    lib = _lib.lib()
    sizes = [1, 2, 37, 511, 512, 513, 4096, (1 << 30) - 1]
    fm = [lib.tzr_wukong_fm_bwd_workspace(b, 27, 128, 24) for b in sizes]
    mix = [lib.tzr_wukong_mix_bwd_workspace(b, 27, 128, 16, 16) for b in sizes]
    for q in (fm, mix):
        assert all(a <= b for a, b in zip(q, q[1:])) and q[0] < q[3] < q[4] == q[5] == q[-1]  # (no more rows than the largest grid)
    assert fm[4] == 512 * 3 * 27 * 24 * 4 + 256 and mix[4] == 512 * (27 * 32 + 27 * 16 + 2 * 128) * 4 + 256
    # outside the limits there is nothing to size: the slack alone
    assert lib.tzr_wukong_fm_bwd_workspace(4, 65, 8, 2) == 256 and lib.tzr_wukong_mix_bwd_workspace(4, 5, 129, 4, 3) == 256


def test_wukong_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_wukong_fm_fwd", "tzr_wukong_fm_bwd_workspace", "tzr_wukong_fm_bwd", "tzr_wukong_mix_fwd", "tzr_wukong_mix_bwd_workspace",
                 "tzr_wukong_mix_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert _lib.ABI_VERSION == 15
