"""Return codes of tzr_mlp2_fwd, tzr_mlp2_bwd, tzr_mlp2_bwd_parts and tzr_mlp_tail (include/tzrec_hip.h, "small dense layer
stacks"): a bad argument comes back as a negative status code, nothing is launched, and the NaN-filled outputs stay as they
were.  Called through ctypes on the emulator build here and on the gfx950 library under `-m gpu`, one valid call per entry first
(the argument order of every refused call is that call's)."""
import ctypes as C

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, LAUNCH, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3, -4
B, K0, H1, H2 = 20, 13, 64, 16
T1, T2 = 64, 32

FWD_ORDER = ("x", "xs", "B", "K0", "Wa", "ba", "H1", "Wb", "bb", "H2", "ha", "has", "hb", "hbs")
BWD_HEAD = ("dhb", "dhbs", "hb", "hbs", "ha", "has", "x", "xs", "B", "K0", "H1", "H2", "Wb")
BWD_ORDER = BWD_HEAD + ("dWa", "dba", "dWb", "dbb", "ws", "wsn")
PARTS_ORDER = BWD_HEAD + ("ws", "wsn", "G", "P")
TAIL_ORDER = ("y1", "y1s", "labels", "isize", "isfloat", "B", "H1", "W2", "b2", "H2", "w3", "b3", "logits", "g1", "g1s", "dW2", "db2", "dw3",
              "scal", "db1", "ws", "wsn")


class Call:
    """one entry point with a full set of valid arguments: `rc(name=value, ...)` calls it with some replaced and checks that
    every output still holds its NaNs when the call was refused"""

    def __init__(self, dev, fn, order, tensors, scalars, outputs):
        self.fn, self.order, self.t, self.s, self.outputs = fn, order, tensors, scalars, outputs
        self.st = _lib.stream_ptr(dev)
        self.dev = dev

    def rc(self, **over):
        a = {k: _lib.ptr(v) for k, v in self.t.items()}
        a.update(self.s)
        a.update(over)
        rc = self.fn(*[a[k] for k in self.order], self.st)
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        if rc != OK:
            assert all(bool(torch.isnan(self.t[k]).all()) for k in self.outputs), "a refused call wrote to its outputs"
        return rc


def _f(dev, *shape, fill=0.5):
    return torch.full(shape, fill, dtype=torch.float32, device=dev)


def _ws(dev):
    n = _lib.lib().tzr_mlp_workspace()
    return _lib.workspace(n, dev), n - 256  # (the bytes the entries ask for behind the 256 of alignment slack)


def _mlp2(dev, which):
    L = _lib.lib()
    nan = float("nan")
    ws, need = _ws(dev)
    t = {"x": _f(dev, B, K0), "Wa": _f(dev, H1, K0), "ba": _f(dev, H1), "Wb": _f(dev, H2, H1), "bb": _f(dev, H2), "ws": ws}
    s = {"xs": K0, "B": B, "K0": K0, "H1": H1, "H2": H2, "has": H1, "hbs": H2, "dhbs": H2, "wsn": need}
    if which == "fwd":
        t.update(ha=_f(dev, B, H1, fill=nan), hb=_f(dev, B, H2, fill=nan))
        return Call(dev, L.tzr_mlp2_fwd, FWD_ORDER, t, s, ("ha", "hb"))
    t.update(ha=_f(dev, B, H1), hb=_f(dev, B, H2), dhb=_f(dev, B, H2))
    if which == "bwd":
        t.update(dWa=_f(dev, H1, K0, fill=nan), dba=_f(dev, H1, fill=nan), dWb=_f(dev, H2, H1, fill=nan), dbb=_f(dev, H2, fill=nan))
        return Call(dev, L.tzr_mlp2_bwd, BWD_ORDER, t, s, ("dWa", "dba", "dWb", "dbb"))
    G, P = C.c_int(-7), C.c_int(-7)
    s.update(G=C.byref(G), P=C.byref(P))
    c = Call(dev, L.tzr_mlp2_bwd_parts, PARTS_ORDER, t, s, ())
    c.G, c.P = G, P
    return c


def _tail(dev, labels=None):
    nan = float("nan")
    ws, need = _ws(dev)
    y = torch.zeros(B, dtype=torch.int64, device=dev) if labels is None else labels.to(dev)
    t = {"y1": _f(dev, B, T1), "labels": y, "W2": _f(dev, T2, T1), "b2": _f(dev, T2), "w3": _f(dev, T2), "b3": _f(dev, 1), "ws": ws,
         "logits": _f(dev, B, fill=nan), "g1": _f(dev, B, T1, fill=nan), "dW2": _f(dev, T2, T1, fill=nan), "db2": _f(dev, T2, fill=nan),
         "dw3": _f(dev, T2, fill=nan), "scal": _f(dev, 2, fill=nan), "db1": _f(dev, T1, fill=nan)}
    s = {"y1s": T1, "g1s": T1, "B": B, "H1": T1, "H2": T2, "isize": y.element_size(), "isfloat": int(y.is_floating_point()), "wsn": need}
    c = Call(dev, _lib.lib().tzr_mlp_tail, TAIL_ORDER, t, s, ("logits", "g1", "dW2", "db2", "dw3", "scal", "db1"))
    return c


def test_mlp2_fwd_return_codes(dev):
    """B = 0 is TZR_OK for the forward (an empty batch is a no-op: nothing to write); the optional biases may be null"""
    c = _mlp2(dev, "fwd")
    for name in ("x", "Wa", "Wb", "ha", "hb"):
        assert c.rc(**{name: None}) == INVALID, name
    assert c.rc(B=-1) == INVALID
    for name in ("K0", "H1", "H2"):
        assert c.rc(**{name: -1}) == INVALID and c.rc(**{name: 0}) == INVALID, name
    assert c.rc(K0=33) == UNSUPPORTED and c.rc(H1=65) == UNSUPPORTED and c.rc(H2=33) == UNSUPPORTED
    assert c.rc(B=0) == OK and c.rc(B=0, K0=33) == UNSUPPORTED
    assert bool(torch.isnan(c.t["ha"]).all()) and bool(torch.isnan(c.t["hb"]).all())  # B = 0 wrote nothing
    assert c.rc(ba=None, bb=None) == OK
    assert not bool(torch.isnan(c.t["ha"]).any()) and not bool(torch.isnan(c.t["hb"]).any())


@pytest.mark.parametrize("which", ["bwd", "parts"])
def test_mlp2_bwd_return_codes(dev, which):
    """B = 0 is TZR_ERR_INVALID for the backward (the code asks for B > 0: a gradient of no samples is not defined as zeros here);
    the bias gradients may be null"""
    c = _mlp2(dev, which)
    for name in ("dhb", "hb", "ha", "x", "Wb") + (("dWa", "dWb") if which == "bwd" else ("G", "P")):
        assert c.rc(**{name: None}) == INVALID, name
    assert c.rc(B=0) == INVALID and c.rc(B=-1) == INVALID
    for name in ("K0", "H1", "H2"):
        assert c.rc(**{name: -1}) == INVALID and c.rc(**{name: 0}) == INVALID, name
    assert c.rc(K0=33) == UNSUPPORTED and c.rc(H1=65) == UNSUPPORTED and c.rc(H2=33) == UNSUPPORTED
    ws, need = _lib.ptr(c.t["ws"]), c.s["wsn"]
    assert c.rc(ws=None) == WORKSPACE and c.rc(ws=None, wsn=0) == WORKSPACE
    assert c.rc(ws=ws + 8) == WORKSPACE  # 8 bytes off the 256-byte alignment
    assert c.rc(wsn=need - 1) == WORKSPACE  # one byte short
    if which == "parts":
        assert (c.G.value, c.P.value) == (-7, -7)  # no refused call wrote the counts
        assert c.rc() == OK and (c.G.value, c.P.value) == (1, H2 * H1 + H2 + H1 * K0 + H1)
    else:
        assert c.rc(dba=None, dbb=None) == OK
        assert bool(torch.isnan(c.t["dba"]).all()) and not bool(torch.isnan(c.t["dWa"]).any()) and not bool(torch.isnan(c.t["dWb"]).any())
        assert c.rc() == OK and not bool(torch.isnan(c.t["dba"]).any()) and not bool(torch.isnan(c.t["dbb"]).any())


def test_mlp_tail_return_codes(dev):
    """B = 0 is TZR_ERR_INVALID for the tail (the loss is a mean over the batch: 1 / B); b2 and b3 may be null"""
    c = _tail(dev)
    for name in ("y1", "labels", "W2", "w3", "logits", "g1", "dW2", "db2", "dw3", "scal", "db1"):
        assert c.rc(**{name: None}) == INVALID, name
    assert c.rc(B=0) == INVALID and c.rc(B=-1) == INVALID
    for name in ("H1", "H2"):
        assert c.rc(**{name: -1}) == INVALID and c.rc(**{name: 0}) == INVALID, name
    assert c.rc(H1=65) == UNSUPPORTED and c.rc(H2=33) == UNSUPPORTED
    ws, need = _lib.ptr(c.t["ws"]), c.s["wsn"]
    assert c.rc(ws=None) == WORKSPACE and c.rc(ws=ws + 8) == WORKSPACE and c.rc(wsn=need - 1) == WORKSPACE
    assert c.rc(b2=None, b3=None) == OK
    assert c.rc() == OK and not any(bool(torch.isnan(c.t[k]).any()) for k in c.outputs)


@pytest.mark.parametrize("knob", [0, -1])
@pytest.mark.parametrize("dtype", [torch.float64, torch.int16])
def test_mlp_tail_refuses_other_label_types(dev, knob, dtype):
    """float64 and int16 labels: TZR_ERR_UNSUPPORTED from the MFMA kernel's launcher (knob 0) and the general kernel's (knob -1)"""
    assert _lib.lib().tzr_tune(b"mlp_mfma", knob) == OK
    c = _tail(dev, labels=torch.zeros(B, dtype=dtype))
    assert c.rc() == UNSUPPORTED
    y32 = torch.zeros(B, dtype=torch.int32, device=dev)
    assert c.rc(isize=4, isfloat=0, labels=_lib.ptr(y32)) == OK
