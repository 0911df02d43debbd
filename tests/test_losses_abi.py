"""Argument checks of the three entry points of csrc/loss_ops.hip: the stated error code, nothing launched, outputs untouched."""
import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
B, C = 70, 5


class _Call:
    """one valid call of `entry`, whose arguments a test replaces by name"""

    def __init__(self, entry, dev):
        self.entry, self.dev = entry, dev
        g = torch.Generator().manual_seed(1)
        width = {"pointwise": (B,), "softmax": (B, C), "jrc": (B, 2)}[entry]
        self.x = torch.randn(*width, generator=g).to(dev)
        self.y = torch.randint(0, 2, (B,), generator=g).to(dev)
        self.sid = torch.randint(0, 9, (B,), generator=g).to(dev)
        self.order = torch.sort(self.sid, stable=True).indices
        self.loss, self.scale = torch.full((), 77.0, device=dev), torch.full((), 77.0, device=dev)
        self.grad = torch.full(width, 77.0, device=dev)
        self.bad = torch.full((), 7, dtype=torch.int64, device=dev)
        L = _lib.lib()
        n = {"pointwise": L.tzr_loss_pointwise_workspace(B), "softmax": L.tzr_softmax_ce_workspace(B, C), "jrc": L.tzr_jrc_loss_workspace(B)}[entry]
        self.ws = _lib.workspace(n, dev)
        self.a = dict(logits=_lib.ptr(self.x), labels=_lib.ptr(self.y), itemsize=8, is_float=0, B=B, C=C, loss=_lib.ptr(self.loss),
                      grad=_lib.ptr(self.grad), scale=_lib.ptr(self.scale), ws=_lib.ptr(self.ws), ws_bytes=self.ws.numel(),
                      sid=_lib.ptr(self.sid), order=_lib.ptr(self.order), kind=0)

    def __call__(self, **over):
        a = {**self.a, **over}
        L, w = _lib.lib(), (None, None, 0, 0, 1.0, 1.0, 1.0)
        s = _lib.stream_ptr(self.dev)
        if self.entry == "pointwise":
            rc = L.tzr_loss_pointwise(a["kind"], 0.0, 0.0, a["logits"], a["labels"], a["itemsize"], a["is_float"], *w, a["B"], a["loss"], a["grad"],
                                      a["scale"], a["ws"], a["ws_bytes"], s)
        elif self.entry == "softmax":
            rc = L.tzr_softmax_ce(a["logits"], a["C"], a["C"], a["labels"], a["itemsize"], a["is_float"], 0.0, *w, a["B"], a["loss"], a["grad"],
                                  a["scale"], _lib.ptr(self.bad), a["ws"], a["ws_bytes"], s)
        else:
            rc = L.tzr_jrc_loss(a["logits"], a["labels"], a["itemsize"], a["is_float"], a["sid"], a["order"], 0.5, *w, a["B"], a["loss"], a["grad"],
                                a["scale"], a["ws"], a["ws_bytes"], s)
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return rc

    def untouched(self):
        return float(self.loss) == 77.0 and float(self.scale) == 77.0 and bool((self.grad == 77.0).all()) and int(self.bad) == 7


@pytest.mark.parametrize("entry", ["pointwise", "softmax", "jrc"])
def test_refusals_leave_the_outputs_untouched(dev, entry):
    call = _Call(entry, dev)
    cases = [(dict(logits=None), INVALID), (dict(labels=None), INVALID), (dict(loss=None), INVALID), (dict(grad=None), INVALID),
             (dict(scale=None), INVALID), (dict(B=0), INVALID), (dict(B=-3), INVALID),
             (dict(ws=None), WORKSPACE), (dict(ws_bytes=call.a["ws_bytes"] - 300), WORKSPACE), (dict(ws=call.a["ws"] + 64), WORKSPACE),
             (dict(itemsize=2), UNSUPPORTED), (dict(itemsize=8, is_float=1), UNSUPPORTED)]
    if entry == "pointwise":
        cases += [(dict(kind=3), INVALID), (dict(kind=-1), INVALID)]
    if entry == "softmax":
        cases += [(dict(C=1), INVALID), (dict(C=0), INVALID), (dict(itemsize=4, is_float=1), UNSUPPORTED)]
    if entry == "jrc":
        cases += [(dict(sid=None), INVALID), (dict(order=None), INVALID)]
    for over, want in cases:
        assert call(**over) == want, (entry, over)
        assert call.untouched(), (entry, over)
    assert call() == OK and not call.untouched()
    assert bool(torch.isfinite(call.loss)) and abs(float(call.scale) - 1.0 / B) < 1e-9
