"""tzr_distill_loss_fwd / _bwd / _workspace at the C boundary: every refusal returns its error code and launches nothing -- the
outputs, pre-filled with a sentinel, are untouched -- and the struct, the limits and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
SENTINEL = 12345.0


class Call:
    """a valid call (B = 5, pairs of widths (8, 12), C = 1, cosine, weights) whose every output holds the sentinel"""

    def __init__(self, dev, B=5, widths=(8, 12), Cn=1, cosine=1):
        f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
        n = max(B, 1)
        self.dev, P = dev, len(widths)
        self.l = [torch.randn(n, max(W, 1)).to(dev) for W in widths]
        self.b = [torch.randn(n, max(W, 1)).to(dev) for W in widths]
        self.ll, self.lb, self.w = torch.randn(n, max(Cn, 1)).to(dev), torch.randn(n, max(Cn, 1)).to(dev), torch.rand(n).to(dev)
        self.g = torch.ones(P + 1, device=dev)
        self.out = {"loss": f(P + 1), "scale": f(1 + _lib.DISTILL_MAX_PAIRS), "dlogits_light": f(n, max(Cn, 1))}
        self.dl = [f(n, max(W, 1)) for W in widths]
        m = self.m = _lib.TzrDistillLoss()
        m.B, m.P, m.C, m.cosine = B, P, Cn, cosine
        for p in range(min(P, _lib.DISTILL_MAX_PAIRS)):
            W = widths[p]
            m.W[p] = W
            m.light[p], m.light_stride[p], m.booster[p], m.booster_stride[p] = self.l[p].data_ptr(), max(W, 1), self.b[p].data_ptr(), max(W, 1)
            m.dlight[p], m.dlight_stride[p], m.grad_sim[p] = self.dl[p].data_ptr(), max(W, 1), self.g.data_ptr() + 4 * p
        m.logits_light, m.logits_booster, m.w = self.ll.data_ptr(), self.lb.data_ptr(), self.w.data_ptr()
        m.grad_hint = self.g.data_ptr() + 4 * P
        for k, t in self.out.items():
            setattr(m, k, t.data_ptr())
        self.ws = _lib.workspace(_lib.lib().tzr_distill_loss_workspace(C.byref(m)), dev)
        m.ws, m.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def set(self, fields):
        """name -> value, "+n" (added to the field's value); name = (array field, index) for an element"""
        for k, v in fields.items():
            if isinstance(k, tuple):
                arr = getattr(self.m, k[0])
                arr[k[1]] = arr[k[1]] + int(v) if isinstance(v, str) else v
            else:
                setattr(self.m, k, getattr(self.m, k) + int(v) if isinstance(v, str) else v)

    def fwd(self):
        return _lib.lib().tzr_distill_loss_fwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def bwd(self):
        return _lib.lib().tzr_distill_loss_bwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def tensors(self):
        return dict(self.out, **{f"dlight{p}": t for p, t in enumerate(self.dl)})

    def untouched(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.tensors().values())


@pytest.mark.parametrize("cosine", [1, 0])
def test_a_valid_call_runs_and_writes(dev, cosine):
    c = Call(dev, cosine=cosine)
    assert c.fwd() == OK and c.bwd() == OK
    for k, t in c.tensors().items():
        keep = slice(0, 3) if k == "scale" else slice(None)  # (scale: B / sum(w) and one entry per pair of the call)
        assert not bool((t[keep] == SENTINEL).any()), k


REFUSALS = {
    "W_not_multiple_of_4": (dict(widths=(8, 6)), {}, UNSUPPORTED),
    "W_below_4": (dict(widths=(0, 8)), {}, UNSUPPORTED),
    "W_above_1024": (dict(widths=(1028,)), {}, UNSUPPORTED),
    "P_9": (dict(widths=(4,) * 9), {}, UNSUPPORTED),
    "P_negative": ({}, dict(P=-1), UNSUPPORTED),
    "C_0": (dict(Cn=0), {}, UNSUPPORTED),
    "C_65": (dict(Cn=65), {}, UNSUPPORTED),
    "B_2_to_the_31": ({}, dict(B=1 << 31), UNSUPPORTED),
    "cosine_not_0_or_1": (dict(cosine=2), {}, UNSUPPORTED),
    "light_stride_odd": ({}, {("light_stride", 0): 9}, UNSUPPORTED),
    "booster_stride_short": ({}, {("booster_stride", 1): 8}, UNSUPPORTED),
    "limits_before_pointers": ({}, {("light", 0): 0, ("W", 1): 6}, UNSUPPORTED),
    "B_negative": ({}, dict(B=-1), INVALID),
    "light_null": ({}, {("light", 1): 0}, INVALID),
    "light_misaligned": ({}, {("light", 0): "+4"}, INVALID),
    "booster_null": ({}, {("booster", 0): 0}, INVALID),
    "booster_misaligned": ({}, {("booster", 1): "+8"}, INVALID),
    "logits_light_null": ({}, dict(logits_light=0), INVALID),
    "logits_booster_misaligned": ({}, dict(logits_booster="+2"), INVALID),
    "w_misaligned": ({}, dict(w="+2"), INVALID),
    "scale_null": ({}, dict(scale=0), INVALID),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_both_entries_refuse_and_launch_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    c.set(fields)
    assert c.fwd() == code and c.bwd() == code, name
    assert c.untouched(), name


FWD_ONLY = {"loss_null": (dict(loss=0), INVALID), "loss_misaligned": (dict(loss="+2"), INVALID), "ws_null": (dict(ws=0), WORKSPACE),
            "ws_misaligned": (dict(ws="+16"), WORKSPACE), "ws_short": (dict(ws_bytes=4), WORKSPACE)}
BWD_ONLY = {"grad_sim_misaligned": ({("grad_sim", 1): "+2"}, INVALID), "grad_hint_misaligned": (dict(grad_hint="+2"), INVALID),
            "dlight_misaligned": ({("dlight", 0): "+4"}, INVALID), "dlogits_light_misaligned": (dict(dlogits_light="+2"), INVALID),
            "dlight_stride_short": ({("dlight_stride", 1): 8}, UNSUPPORTED), "dlight_stride_odd": ({("dlight_stride", 0): 9}, UNSUPPORTED)}


@pytest.mark.parametrize("name", sorted(FWD_ONLY))
def test_the_forward_refuses(dev, name):
    fields, code = FWD_ONLY[name]
    c = Call(dev)
    c.set(fields)
    assert c.fwd() == code and c.untouched(), name


@pytest.mark.parametrize("name", sorted(BWD_ONLY))
def test_the_backward_refuses(dev, name):
    fields, code = BWD_ONLY[name]
    c = Call(dev)
    assert c.fwd() == OK
    before = {k: v.clone() for k, v in c.tensors().items()}
    c.set(fields)
    assert c.bwd() == code, name
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(torch.equal(before[k], t) for k, t in c.tensors().items()), name  # (the gradients still hold the sentinel)


def test_null_outputs_and_gradients_are_skipped_or_zero(dev):
    """dlight[p] == 0: the pair is skipped; grad_sim[p] == 0 with dlight[p]: zero rows; the same for the hint"""
    c = Call(dev)
    c.set({("dlight", 0): 0, ("grad_sim", 1): 0, "grad_hint": 0})
    assert c.fwd() == OK and c.bwd() == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((c.dl[0] == SENTINEL).all()) and float(c.dl[1].abs().max()) == 0.0 and float(c.out["dlogits_light"].abs().max()) == 0.0
    c = Call(dev)
    c.set({"dlogits_light": 0})
    assert c.fwd() == OK and c.bwd() == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert bool((c.out["dlogits_light"] == SENTINEL).all()) and not bool((c.dl[1] == SENTINEL).any())


def test_an_empty_batch_is_ok_without_a_launch(dev):
    c = Call(dev, B=0)
    assert c.fwd() == OK and c.bwd() == OK and c.untouched()


def test_null_struct_and_workspace_query(dev):
    L = _lib.lib()
    assert L.tzr_distill_loss_fwd(None, None) == INVALID and L.tzr_distill_loss_bwd(None, None) == INVALID
    assert L.tzr_distill_loss_workspace(None) == 256
    c = Call(dev, B=67)
    assert L.tzr_distill_loss_workspace(C.byref(c.m)) == 512 + 256  # seventeen workgroups of four sums: 68 floats, rounded up, plus the slack


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    assert C.sizeof(_lib.TzrDistillLoss) == 576 and _lib.ABI_VERSION == 15
    assert "#define TZR_DISTILL_MAX_PAIRS 8" in header and _lib.DISTILL_MAX_PAIRS == 8
    assert "#define TZR_DISTILL_MAX_W 1024" in header and _lib.DISTILL_MAX_W == 1024
    for name in ("tzr_distill_loss_workspace", "tzr_distill_loss_fwd", "tzr_distill_loss_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    fields = [n for n, _ in _lib.TzrDistillLoss._fields_]
    body = header[header.index("typedef struct TzrDistillLoss {"):header.index("} TzrDistillLoss;")]
    pos = [body.index(f" {n}[") if f" {n}[" in body else body.index(f" {n};") for n in fields if n not in ("P", "C", "cosine", "pad_")]
    assert pos == sorted(pos) and "int32_t P, C, cosine, pad_;" in body  # the same order
