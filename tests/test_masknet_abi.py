"""Error behaviour of tzr_ln_mask_fwd / tzr_ln_mask_bwd_workspace / tzr_ln_mask_bwd (csrc/ln_mask.hip), as tests/test_cross_net_abi.py
checks their siblings: bad arguments come back as negative status codes -- never a crash, never a launch -- and B == 0 is a TZR_OK
no-op that writes nothing."""
import ctypes as C
import os

import torch

from torcheasyrec_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -4
B, D, N = 3, 10, 2
S = D + 2  # row stride of every tensor below


def test_ln_mask_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    mk = lambda: [torch.ones(B, S, dtype=torch.float32, device=dev) for _ in range(9)]  # (room for 9 outputs: the n_out = 9 case is refused before any is read)
    x, m, out, gout, gx, gm = mk(), mk(), mk(), mk(), mk(), mk()
    gamma = [torch.full((D,), 1.5, dtype=torch.float32, device=dev) for _ in range(9)]
    beta = [torch.full((D,), 0.2, dtype=torch.float32, device=dev) for _ in range(9)]
    stats = torch.zeros(B, 9, 2, dtype=torch.float32, device=dev)
    dg, db = (torch.zeros(9, D, dtype=torch.float32, device=dev) for _ in range(2))
    need = lib.tzr_ln_mask_bwd_workspace(B, D, N, 0)
    ws = _lib.workspace(lib.tzr_ln_mask_bwd_workspace(B, D, 8, 0), dev)
    # one row [dgamma | dbeta] per workgroup and grid slice (+ slack); a shared x needs one slice whatever n_out
    assert need >= N * 2 * D * 4 + 256 and lib.tzr_ln_mask_bwd_workspace(B, D, N, 1) < need < lib.tzr_ln_mask_bwd_workspace(B, D, 8, 0)
    assert lib.tzr_ln_mask_bwd_workspace(B, D, 8, 1) == lib.tzr_ln_mask_bwd_workspace(B, D, N, 1)

    def arr(ts):
        return (C.c_void_p * len(ts))(*[p(t) for t in ts])

    def strides(n=9, s=S):
        return (C.c_int64 * n)(*([s] * n))

    written = out + gx + gm + [stats, dg, db]

    def fwd(x_=arr(x), xs=strides(), g_=arr(gamma), b_=arr(beta), m_=arr(m), ms=strides(), o_=arr(out), os_=strides(), n=N, shared=0, relu=1,
            nb=B, d=D, st_=p(stats)):
        return lib.tzr_ln_mask_fwd(x_, xs, g_, b_, m_, ms, o_, os_, n, shared, relu, 1e-5, nb, d, st_, None)

    def bwd(go_=arr(gout), gs=strides(), x_=arr(x), xs=strides(), g_=arr(gamma), b_=arr(beta), m_=arr(m), ms=strides(), st_=p(stats), n=N,
            shared=0, relu=1, nb=B, d=D, gx_=arr(gx), gxs=strides(), gm_=arr(gm), gms=strides(), dg_=p(dg), db_=p(db), ws_=p(ws),
            wsn=ws.numel()):
        return lib.tzr_ln_mask_bwd(go_, gs, x_, xs, g_, b_, m_, ms, st_, n, shared, relu, nb, d, gx_, gxs, gm_, gms, dg_, db_, ws_, wsn, None)

    assert fwd() == OK and bwd() == OK
    assert fwd(shared=1) == OK and bwd(shared=1) == OK and fwd(n=8) == OK and bwd(n=8) == OK
    assert fwd(m_=None, ms=None) == OK and bwd(m_=None, ms=None, gm_=None, gms=None) == OK  # (no masks)
    assert fwd(xs=strides(s=D), ms=strides(s=D), os_=strides(s=D)) == OK

    def snapshot():
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return [t.clone() for t in written]

    for t in written:
        t.fill_(7.0)
    before = snapshot()
    hole = (C.c_void_p * N)(p(x[0]), None)  # an output without a tensor
    for fn, names in ((fwd, ("x_", "xs", "g_", "b_", "o_", "os_", "st_")),
                      (bwd, ("go_", "gs", "x_", "xs", "g_", "b_", "st_", "gx_", "gxs", "gm_", "gms", "dg_", "db_", "ws_"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name  # null pointer
        assert fn(x_=hole) == INVALID and fn(g_=hole) == INVALID and fn(b_=hole) == INVALID and fn(m_=hole) == INVALID
        assert fn(nb=-1) == INVALID and fn(d=0) == INVALID and fn(d=-3) == INVALID and fn(n=0) == INVALID and fn(n=-1) == INVALID
        assert fn(d=1025) == UNSUPPORTED and fn(n=9) == UNSUPPORTED
        assert fn(xs=strides(s=D - 1)) == UNSUPPORTED and fn(ms=strides(s=D - 1)) == UNSUPPORTED  # a stride below D
    assert fwd(os_=strides(s=D - 1)) == UNSUPPORTED and bwd(gs=strides(s=D - 1)) == UNSUPPORTED
    assert bwd(gxs=strides(s=D - 1)) == UNSUPPORTED and bwd(gms=strides(s=D - 1)) == UNSUPPORTED
    assert bwd(ws_=p(ws) + 4) == INVALID  # a misaligned workspace
    assert bwd(wsn=need - 256 - 4) == UNSUPPORTED and bwd(wsn=0) == UNSUPPORTED  # a workspace that is too small
    # no sample: nothing is launched, nothing is read or written
    assert fwd(nb=0) == OK and bwd(nb=0) == OK
    assert fwd(nb=0, x_=None, g_=None, b_=None, m_=None, o_=None, st_=None) == OK
    assert bwd(nb=0, go_=None, x_=None, g_=None, b_=None, m_=None, st_=None, gx_=None, gm_=None, dg_=None, db_=None, ws_=None, wsn=0) == OK
    for a, b in zip(before, snapshot()):
        assert torch.equal(a, b)
    assert bwd(wsn=need - 256) == OK  # (the query's 256 bytes are the room to align in)


def test_ln_mask_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_ln_mask_fwd", "tzr_ln_mask_bwd_workspace", "tzr_ln_mask_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert _lib.ABI_VERSION == 15
