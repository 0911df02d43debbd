"""Error behaviour of tzr_cin_fwd / tzr_cin_bwd_workspace / tzr_cin_bwd (csrc/cin.hip), as tests/test_cross_net_abi.py checks
their siblings: bad arguments come back as negative status codes -- never a crash, never a launch, the outputs untouched --
and B == 0 is a TZR_OK no-op that writes nothing."""
import ctypes as C
import os

import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
B, F, D, LAYERS = 3, 4, 6, [5, 3]
TOTAL = 5 * 16 + 5 + 3 * 20 + 3


class _Args:
    def __init__(self, dev):
        p, f32 = _lib.ptr, dict(dtype=torch.float32, device=dev)
        self.lib, self.dev = _lib.lib(), dev
        self.x, self.gx = torch.ones(B, F * D + 2, **f32), torch.full((B, F * D + 2), 7.0, **f32)
        self.y, self.gy = torch.full((B, 12), 7.0, **f32), torch.ones(B, 12, **f32)  # (room for the four layers of one call)
        self.w = [torch.full((o, h * F, 1), 0.1, **f32) for o, h in ((5, 4), (3, 5), (2, 3), (2, 2), (2, 2))]
        self.c = [torch.full((o,), 0.2, **f32) for o in (5, 3, 2, 2, 2)]
        self.xs = [torch.full((B, 5, D), 7.0, **f32)] + [torch.full((B, 3, D), 7.0, **f32) for _ in range(3)]
        self.dwc = torch.full((TOTAL + 64,), 7.0, **f32)
        self.need = self.lib.tzr_cin_bwd_workspace(B, F, D, self.sizes(LAYERS), 2)
        self.ws = _lib.workspace(self.need, dev)
        self.outputs = (self.y, self.gx, self.dwc, *self.xs)

    @staticmethod
    def sizes(layers):
        return (C.c_int * len(layers))(*layers)

    def arr(self, ts):
        return (C.c_void_p * len(ts))(*[_lib.ptr(t) for t in ts])

    def fwd(self, **k):
        p = _lib.ptr
        a = dict(x=p(self.x), xs_=F * D + 2, w=self.arr(self.w), c=self.arr(self.c), layers=LAYERS, n=B, f=F, d=D, xs=self.arr(self.xs), y=p(self.y), ys=12)
        a.update(k)
        sizes = self.sizes(a["layers"]) if a["layers"] is not None else None
        L = a.get("l", len(a["layers"]) if a["layers"] is not None else 2)
        return self.lib.tzr_cin_fwd(a["x"], a["xs_"], a["w"], a["c"], sizes, L, a["n"], a["f"], a["d"], a["xs"], a["y"], a["ys"], None)

    def bwd(self, **k):
        p = _lib.ptr
        a = dict(gy=p(self.gy), gs=12, x=p(self.x), xs_=F * D + 2, w=self.arr(self.w), layers=LAYERS, n=B, f=F, d=D, xs=self.arr(self.xs),
                 gx=p(self.gx), gxs=F * D + 2, dwc=p(self.dwc), ws=p(self.ws), wsn=self.ws.numel())
        a.update(k)
        sizes = self.sizes(a["layers"]) if a["layers"] is not None else None
        L = a.get("l", len(a["layers"]) if a["layers"] is not None else 2)
        return self.lib.tzr_cin_bwd(a["gy"], a["gs"], a["x"], a["xs_"], a["w"], sizes, L, a["n"], a["f"], a["d"], a["xs"], a["gx"], a["gxs"],
                                    a["dwc"], a["ws"], a["wsn"], None)

    def untouched(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return all(float((t - 7.0).abs().max()) == 0.0 for t in self.outputs)


def test_cin_runs_and_takes_the_optional_arguments(dev):
    a = _Args(dev)
    assert a.fwd() == OK and a.bwd() == OK
    assert not a.untouched()
    assert a.fwd(xs=None) == OK  # (inference: nothing is saved)
    assert a.fwd(layers=[5], xs=None, ys=5) == OK and a.fwd(layers=[5, 3, 2, 2], ys=12) == OK
    assert a.bwd(wsn=a.need - 256) == OK  # (the query's 256 bytes are the room to align in)


def test_cin_invalid_arguments_leave_the_outputs_alone(dev):
    a = _Args(dev)
    hole_w = (C.c_void_p * 2)(_lib.ptr(a.w[0]), None)
    hole_xs = (C.c_void_p * 1)(None)
    for fn, names in ((a.fwd, ("x", "w", "c", "y", "layers")), (a.bwd, ("gy", "x", "w", "xs", "gx", "dwc", "layers"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name  # null pointer
        assert fn(w=hole_w) == INVALID  # a layer without a parameter
        assert fn(n=-1) == INVALID and fn(f=0) == INVALID and fn(d=0) == INVALID and fn(d=-3) == INVALID
        assert fn(layers=[5, 0]) == INVALID and fn(layers=[-1, 3]) == INVALID and fn(layers=[], l=0) == INVALID and fn(l=-1) == INVALID
    assert a.fwd(c=hole_w) == INVALID and a.bwd(xs=hole_xs) == INVALID
    assert a.untouched()


def test_cin_unsupported_arguments_leave_the_outputs_alone(dev):
    a = _Args(dev)
    for fn in (a.fwd, a.bwd):
        assert fn(d=65) == UNSUPPORTED
        assert fn(layers=[257, 3]) == UNSUPPORTED and fn(layers=[5, 3, 2, 2, 2]) == UNSUPPORTED
        assert fn(n=1 << 30) == UNSUPPORTED
        assert fn(xs_=F * D - 1) == UNSUPPORTED  # a stride below F D
    assert a.fwd(f=65, xs_=65 * D) == UNSUPPORTED and a.bwd(f=65, xs_=65 * D, gxs=65 * D) == UNSUPPORTED
    assert a.fwd(ys=7) == UNSUPPORTED and a.bwd(gs=7) == UNSUPPORTED and a.bwd(gxs=F * D - 1) == UNSUPPORTED  # below sum O = 8, below F D
    assert a.untouched()


def test_cin_workspace_errors_leave_the_outputs_alone(dev):
    a = _Args(dev)
    assert a.bwd(ws=None) == WORKSPACE and a.bwd(ws=_lib.ptr(a.ws) + 4) == WORKSPACE  # null, misaligned
    assert a.bwd(wsn=a.need - 256 - 4) == WORKSPACE and a.bwd(wsn=0) == WORKSPACE  # short
    assert a.untouched()


def test_cin_empty_batch_is_ok_without_a_launch(dev):
    a = _Args(dev)
    assert a.fwd(n=0) == OK and a.bwd(n=0) == OK
    assert a.fwd(n=0, x=None, y=None, w=None, c=None, xs=None) == OK
    assert a.bwd(n=0, gy=None, x=None, w=None, xs=None, gx=None, dwc=None, ws=None, wsn=0) == OK
    assert a.untouched()


def test_cin_workspace_query_is_monotone_in_the_batch(dev):
    lib, sizes = _lib.lib(), _Args.sizes([128, 128])
    got = [lib.tzr_cin_bwd_workspace(b, 26, 16, sizes, 2) for b in (0, 1, 100, 512, 513, 1024, 1500, 2048, 8192, 1 << 20)]
    one = (128 * 26 * 26 + 128 + 128 * 128 * 26 + 128) * 4
    assert got == sorted(got) and got[0] >= one + 256 and got[-1] <= 8 * one + 256 and got[-1] > got[0]  # (a few parts per layer)
    assert lib.tzr_cin_bwd_workspace(8, 26, 65, sizes, 2) == 256 and lib.tzr_cin_bwd_workspace(8, 26, 16, None, 2) == 256  # (no kernel: no need)


def test_cin_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_cin_fwd", "tzr_cin_bwd_workspace", "tzr_cin_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert _lib.ABI_VERSION == 15
