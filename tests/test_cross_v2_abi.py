"""Error behaviour of tzr_cross_v2_fwd / tzr_cross_v2_bwd_workspace / tzr_cross_v2_bwd (csrc/cross_v2.hip), as
tests/test_cross_net_abi.py checks their v1 siblings: bad arguments come back as negative status codes -- never a crash,
never a launch -- and B == 0 is a TZR_OK no-op that writes nothing."""
import ctypes as C
import os

import torch

from torcheasyrec_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -4
B, D, R, L = 3, 10, 4, 2
SENTINEL = 7.0


def test_cross_v2_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    x, gy, y, dx = (torch.ones(B, D + 2, dtype=torch.float32, device=dev) for _ in range(4))
    xs = torch.zeros(7, B, D, dtype=torch.float32, device=dev)  # (room for the saved tensors of 8 layers)
    t = torch.zeros(8, B, R, dtype=torch.float32, device=dev)
    u = [torch.full((R, D), 0.1, dtype=torch.float32, device=dev) for _ in range(8)]
    v = [torch.full((D, R), 0.2, dtype=torch.float32, device=dev) for _ in range(8)]
    c = [torch.full((D,), 0.3, dtype=torch.float32, device=dev) for _ in range(8)]
    du, dv, dc = (torch.zeros(8, *s, dtype=torch.float32, device=dev) for s in ((R, D), (D, R), (D,)))
    need = lib.tzr_cross_v2_bwd_workspace(B, D, R, L)
    ws = _lib.workspace(need, dev)
    assert need == L * B * (D + R) * 4 + 256 and lib.tzr_cross_v2_bwd_workspace(B, D, R, 8) > need  # dy_l [L, B, D] and dt_l [L, B, R] (+ slack)
    assert lib.tzr_cross_v2_bwd_workspace(B, D + 1, R, L) > need and lib.tzr_cross_v2_bwd_workspace(B, D, R + 1, L) > need

    def arr(ts):
        return (C.c_void_p * len(ts))(*[p(t_) for t_ in ts])

    def fwd(x_=p(x), xs_=D + 2, u_=arr(u), v_=arr(v), c_=arr(c), l=L, n=B, d=D, r=R, y_=p(y), ys=D + 2, sx_=p(xs), st_=p(t)):
        return lib.tzr_cross_v2_fwd(x_, xs_, u_, v_, c_, l, n, d, r, y_, ys, sx_, st_, None)

    def bwd(g_=p(gy), gs=D + 2, x_=p(x), xs_=D + 2, sx_=p(xs), st_=p(t), u_=arr(u), v_=arr(v), c_=arr(c), l=L, n=B, d=D, r=R, dx_=p(dx),
            dxs=D + 2, du_=p(du), dv_=p(dv), dc_=p(dc), ws_=p(ws), wsn=ws.numel()):
        return lib.tzr_cross_v2_bwd(g_, gs, x_, xs_, sx_, st_, u_, v_, c_, l, n, d, r, dx_, dxs, du_, dv_, dc_, ws_, wsn, None)

    y.fill_(SENTINEL), dx.fill_(SENTINEL), du.fill_(SENTINEL), dv.fill_(SENTINEL), dc.fill_(SENTINEL)

    def untouched():
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return all(float((t_ - SENTINEL).abs().max()) == 0.0 for t_ in (y, dx, du, dv, dc))

    hole = (C.c_void_p * L)(p(u[0]), None)  # a layer without a parameter
    for fn, names in ((fwd, ("x_", "u_", "v_", "c_", "y_")),
                      (bwd, ("g_", "x_", "sx_", "st_", "u_", "v_", "c_", "dx_", "du_", "dv_", "dc_", "ws_"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name  # null pointer
        assert fn(u_=hole) == INVALID and fn(v_=hole) == INVALID and fn(c_=hole) == INVALID
        assert fn(n=-1) == INVALID and fn(d=0) == INVALID and fn(d=-3) == INVALID and fn(r=0) == INVALID and fn(r=-1) == INVALID
        assert fn(l=0) == INVALID and fn(l=-1) == INVALID
        assert fn(d=1025, xs_=1025) == UNSUPPORTED and fn(r=65) == UNSUPPORTED and fn(l=9) == UNSUPPORTED
        assert fn(xs_=D - 1) == UNSUPPORTED  # a stride below D
    assert fwd(ys=D - 1) == UNSUPPORTED and bwd(gs=D - 1) == UNSUPPORTED and bwd(dxs=D - 1) == UNSUPPORTED
    assert bwd(wsn=need - 256 - 1) == UNSUPPORTED and bwd(wsn=0) == UNSUPPORTED  # a workspace one byte short, and none
    assert bwd(ws_=p(ws) + 4) == INVALID and bwd(ws_=p(ws) + 128) == INVALID  # a misaligned workspace
    # no sample: nothing is launched, nothing is read or written
    assert fwd(n=0) == OK and bwd(n=0) == OK
    assert fwd(n=0, x_=None, y_=None, u_=None, v_=None, c_=None, sx_=None, st_=None) == OK
    assert bwd(n=0, g_=None, x_=None, sx_=None, st_=None, dx_=None, du_=None, dv_=None, dc_=None, ws_=None, wsn=0) == OK
    assert untouched()  # none of the calls above launched anything
    # the good calls
    assert fwd() == OK and bwd() == OK and fwd(sx_=None, st_=None) == OK  # (the saved tensors are optional in the forward: inference)
    assert bwd(wsn=need - 256) == OK  # (the query's 256 bytes are the room to align in)
    assert fwd(xs_=D, ys=D) == OK and fwd(l=8) == OK and bwd(l=8, ws_=p(big := _lib.workspace(lib.tzr_cross_v2_bwd_workspace(B, D, R, 8), dev)),
                                                           wsn=big.numel()) == OK
    assert fwd(l=1, sx_=None) == OK and bwd(l=1, sx_=None) == OK  # (one layer saves no x_l)
    assert not untouched()


def test_cross_v2_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_cross_v2_fwd", "tzr_cross_v2_bwd_workspace", "tzr_cross_v2_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert _lib.ABI_VERSION == 15
