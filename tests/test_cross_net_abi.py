"""Error behaviour of tzr_cross_fwd / tzr_cross_bwd_workspace / tzr_cross_bwd (csrc/cross_net.hip), as
tests/test_jagged_encoders_abi.py checks their siblings: bad arguments come back as negative status codes -- never a crash,
never a launch -- and B == 0 is a TZR_OK no-op that writes nothing."""
import ctypes as C

import torch

from torcheasyrec_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -4
B, D, L = 3, 10, 2


def test_cross_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    x, gy, y, dx = (torch.ones(B, D + 2, dtype=torch.float32, device=dev) for _ in range(4))
    s = torch.zeros(B, 8, dtype=torch.float32, device=dev)  # (room for the scalars of 8 layers)
    w = [torch.full((1, D), 0.1, dtype=torch.float32, device=dev) for _ in range(8)]
    b = [torch.full((D,), 0.2, dtype=torch.float32, device=dev) for _ in range(8)]
    dw, db = (torch.zeros(8, D, dtype=torch.float32, device=dev) for _ in range(2))
    need = lib.tzr_cross_bwd_workspace(B, D, L)
    ws = _lib.workspace(need, dev)
    assert need >= (3 * D + 2) * 4 + 256 and lib.tzr_cross_bwd_workspace(B, D, 8) > need  # >= one row [A_0 A_1 G | T_0 T_1] (+ slack)

    def arr(ts, n=None):
        return (C.c_void_p * len(ts))(*[p(t) for t in ts[:len(ts) if n is None else n]])

    def fwd(x_=p(x), xs=D + 2, w_=arr(w), b_=arr(b), l=L, n=B, d=D, y_=p(y), ys=D + 2, s_=p(s)):
        return lib.tzr_cross_fwd(x_, xs, w_, b_, l, n, d, y_, ys, s_, None)

    def bwd(g_=p(gy), gs=D + 2, x_=p(x), xs=D + 2, s_=p(s), w_=arr(w), b_=arr(b), l=L, n=B, d=D, dx_=p(dx), dxs=D + 2, dw_=p(dw),
            db_=p(db), ws_=p(ws), wsn=ws.numel()):
        return lib.tzr_cross_bwd(g_, gs, x_, xs, s_, w_, b_, l, n, d, dx_, dxs, dw_, db_, ws_, wsn, None)

    assert fwd() == OK and bwd() == OK and fwd(s_=None) == OK  # (the scalars are optional in the forward: inference)
    assert fwd(xs=D, ys=D) == OK and fwd(l=8) == OK
    hole = (C.c_void_p * L)(p(w[0]), None)  # a layer without a parameter
    for fn, names in ((fwd, ("x_", "w_", "b_", "y_")), (bwd, ("g_", "x_", "s_", "w_", "b_", "dx_", "dw_", "db_", "ws_"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name  # null pointer
        assert fn(w_=hole) == INVALID and fn(b_=hole) == INVALID
        assert fn(n=-1) == INVALID and fn(d=0) == INVALID and fn(d=-3) == INVALID and fn(l=0) == INVALID and fn(l=-1) == INVALID
        assert fn(d=1025, xs=1025) == UNSUPPORTED and fn(l=9) == UNSUPPORTED
        assert fn(xs=D - 1) == UNSUPPORTED  # a stride below D
    assert fwd(ys=D - 1) == UNSUPPORTED and bwd(gs=D - 1) == UNSUPPORTED and bwd(dxs=D - 1) == UNSUPPORTED
    assert bwd(wsn=need - 256 - 4) == UNSUPPORTED and bwd(wsn=0) == UNSUPPORTED  # a workspace that is too small
    assert bwd(wsn=need - 256) == OK  # (the query's 256 bytes are the room to align in)
    # no sample: nothing is launched, nothing is read or written
    y.fill_(7.0), dx.fill_(7.0), dw.fill_(7.0), db.fill_(7.0)
    assert fwd(n=0) == OK and bwd(n=0) == OK
    assert fwd(n=0, x_=None, y_=None, w_=None, b_=None) == OK and bwd(n=0, g_=None, x_=None, s_=None, dx_=None, dw_=None, db_=None, ws_=None, wsn=0) == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for t in (y, dx, dw, db):
        assert float((t - 7.0).abs().max()) == 0.0


def test_cross_symbols_are_declared_and_bound():
    import os

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_cross_fwd", "tzr_cross_bwd_workspace", "tzr_cross_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert _lib.ABI_VERSION == 15
