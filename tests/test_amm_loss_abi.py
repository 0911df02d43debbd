"""tzr_amm_loss_fwd / _bwd / _workspace at the C boundary: every refusal returns its error code and launches nothing -- the
outputs, pre-filled with a sentinel, are untouched -- and the struct, the limit and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
SENTINEL = 12345.0


class Call:
    """a valid call (B = 5, M = 9, D = 8, cosine, weights) whose every output holds the sentinel"""

    def __init__(self, dev, B=5, M=9, D=8, cosine=1):
        f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
        r = lambda n: torch.randn(max(n, 1), D).to(dev)  # noqa: E731
        self.dev = dev
        self.ua, self.ia, self.ue, self.ie, self.w = r(B), r(M), r(B), r(M), torch.rand(max(B, 1)).to(dev)
        self.g = torch.ones(2, device=dev)
        self.out = {"loss": f(2), "rows": f(6, max(B, 1)), "scale": f(1), "dua": f(max(B, 1), D), "dia": f(max(M, 1), D)}
        m = self.m = _lib.TzrAmmLoss()
        m.B, m.M, m.D, m.cosine, m.c_u, m.c_i = B, M, D, cosine, 0.5, 0.5
        for k in ("ua", "ia", "ue", "ie"):
            setattr(m, k, getattr(self, k).data_ptr())
            setattr(m, k + "_stride", D)
        m.w = self.w.data_ptr()
        for k, t in self.out.items():
            setattr(m, k, t.data_ptr())
        m.dua_stride, m.dia_stride, m.grad_u, m.grad_i = D, D, self.g.data_ptr(), self.g.data_ptr() + 4
        self.ws = _lib.workspace(_lib.lib().tzr_amm_loss_workspace(C.byref(m)), dev)
        m.ws, m.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def set(self, fields):
        for k, v in fields.items():
            setattr(self.m, k, getattr(self.m, k) + int(v) if isinstance(v, str) else v)

    def fwd(self):
        return _lib.lib().tzr_amm_loss_fwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def bwd(self):
        return _lib.lib().tzr_amm_loss_bwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def untouched(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.out.values())


def test_a_valid_call_runs_and_writes(dev):
    c = Call(dev)
    assert c.fwd() == OK and c.bwd() == OK
    for k, t in c.out.items():
        assert not bool((t == SENTINEL).any()), k
    assert float(c.out["dia"][5:].abs().max()) == 0.0


REFUSALS = {
    "D_not_multiple_of_4": (dict(D=6), {}, UNSUPPORTED),
    "D_below_4": (dict(D=2), {}, UNSUPPORTED),
    "D_above_256": (dict(D=260), {}, UNSUPPORTED),
    "M_below_B": (dict(B=5, M=4), {}, UNSUPPORTED),
    "B_2_to_the_31": ({}, dict(B=1 << 31, M=1 << 31), UNSUPPORTED),
    "cosine_not_0_or_1": (dict(cosine=2), {}, UNSUPPORTED),
    "ua_stride_odd": ({}, dict(ua_stride=9), UNSUPPORTED),
    "ia_stride_short": ({}, dict(ia_stride=4), UNSUPPORTED),
    "ue_stride_short": ({}, dict(ue_stride=4), UNSUPPORTED),
    "ie_stride_odd": ({}, dict(ie_stride=10), UNSUPPORTED),
    "B_negative": ({}, dict(B=-1), INVALID),
    "ua_null": ({}, dict(ua=0), INVALID),
    "ia_misaligned": ({}, dict(ia="+4"), INVALID),
    "ue_null": ({}, dict(ue=0), INVALID),
    "ie_misaligned": ({}, dict(ie="+8"), INVALID),
    "w_misaligned": ({}, dict(w="+2"), INVALID),
    "rows_null": ({}, dict(rows=0), INVALID),
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
BWD_ONLY = {"grad_u_misaligned": (dict(grad_u="+2"), INVALID), "dua_null": (dict(dua=0), INVALID), "dia_misaligned": (dict(dia="+4"), INVALID),
            "dua_stride_short": (dict(dua_stride=4), UNSUPPORTED), "dia_stride_odd": (dict(dia_stride=9), UNSUPPORTED)}


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
    before = {k: v.clone() for k, v in c.out.items()}
    c.set(fields)
    assert c.bwd() == code, name
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(torch.equal(before[k], c.out[k]) for k in before), name  # (dua, dia still hold the sentinel)


def test_an_empty_batch_is_ok_without_a_launch(dev):
    c = Call(dev, B=0, M=4)
    assert c.fwd() == OK and c.bwd() == OK and c.untouched()


def test_null_struct_and_workspace_query(dev):
    L = _lib.lib()
    assert L.tzr_amm_loss_fwd(None, None) == INVALID and L.tzr_amm_loss_bwd(None, None) == INVALID
    assert L.tzr_amm_loss_workspace(None) == 256
    c = Call(dev, B=67, M=67)
    assert L.tzr_amm_loss_workspace(C.byref(c.m)) == 256 + 256  # seventeen workgroups: 51 floats, rounded up, plus the slack


def test_struct_limit_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    assert C.sizeof(_lib.TzrAmmLoss) == 192 and _lib.ABI_VERSION == 15
    assert "#define TZR_AMM_MAX_D 256" in header and _lib.AMM_MAX_D == 256
    for name in ("tzr_amm_loss_workspace", "tzr_amm_loss_fwd", "tzr_amm_loss_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    fields = [n for n, _ in _lib.TzrAmmLoss._fields_]
    body = header[header.index("typedef struct TzrAmmLoss {"):header.index("} TzrAmmLoss;")]
    pos = [body.index(f" {n}") for n in fields if n not in ("M", "cosine", "c_i")]
    assert pos == sorted(pos)  # the same order
