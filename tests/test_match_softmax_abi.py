"""tzr_match_softmax_fwd / _bwd / _workspace at the C boundary: every refusal returns its error code and launches nothing --
the outputs, pre-filled with a sentinel, are untouched -- and the struct, the limits and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
SENTINEL = 12345.0


class Call:
    """a valid SAMPLED call (B = 5, N = 4, D = 8, cosine) whose every output holds the sentinel"""

    def __init__(self, dev, B=5, M=9, D=8, mode=_lib.MATCH_SAMPLED, cosine=1):
        f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
        self.dev, self.B, self.M, self.D = dev, B, M, D
        self.u, self.v, self.w = torch.randn(max(B, 1), D).to(dev), torch.randn(max(M, 1), D).to(dev), torch.rand(max(B, 1)).to(dev)
        self.out = {"loss": f(1), "lse": f(max(B, 1)), "rmax": f(max(B, 1)), "lsum": f(max(B, 1)), "pos": f(max(B, 1)), "scale": f(1),
                    "rank": torch.full((max(B, 1),), 777, dtype=torch.int32, device=dev),
                    "ru": f(max(B, 1)).double(), "rv": f(max(M, 1)).double(), "sim": f(max(B, 1), max(M, 1) + 1),
                    "du": f(max(B, 1), D), "dv": f(max(M, 1), D)}
        self.g = torch.ones(1, device=dev)
        m = self.m = _lib.TzrMatchSoftmax()
        m.B, m.M, m.D, m.mode, m.cosine, m.inv_temperature = B, M, D, mode, cosine, 20.0
        m.u, m.u_stride, m.v, m.v_stride, m.w = self.u.data_ptr(), D, self.v.data_ptr(), D, self.w.data_ptr()
        for k in ("loss", "lse", "rmax", "lsum", "pos", "scale", "rank", "ru", "rv", "sim", "du", "dv"):
            setattr(m, k, self.out[k].data_ptr())
        m.sim_stride, m.du_stride, m.dv_stride, m.grad_loss = self.out["sim"].stride(0), D, D, self.g.data_ptr()
        self.ws = _lib.workspace(_lib.lib().tzr_match_softmax_workspace(C.byref(m)), dev)
        m.ws, m.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def fwd(self):
        return _lib.lib().tzr_match_softmax_fwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def bwd(self):
        return _lib.lib().tzr_match_softmax_bwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def untouched(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return all(bool((t == (777 if t.dtype == torch.int32 else SENTINEL)).all()) for t in self.out.values())


def test_a_valid_call_runs_and_writes(dev):
    c = Call(dev)
    assert c.fwd() == OK and c.bwd() == OK
    for k in ("loss", "lse", "rmax", "lsum", "pos", "scale", "rank", "ru", "rv", "du", "dv"):
        assert not bool((c.out[k] == (777 if k == "rank" else SENTINEL)).any()), k
    assert bool((c.out["sim"][:, :5] != SENTINEL).all()) and bool((c.out["sim"][:, 5:] == SENTINEL).all())


REFUSALS = {
    "D_not_multiple_of_4": (dict(D=6), {}, UNSUPPORTED),
    "D_below_4": (dict(D=2), {}, UNSUPPORTED),
    "D_above_256": (dict(D=260), {}, UNSUPPORTED),
    "B_zero": (dict(B=0, M=4), {}, UNSUPPORTED),
    "N_negative": (dict(B=5, M=4), {}, UNSUPPORTED),
    "in_batch_M_not_B": (dict(mode=_lib.MATCH_IN_BATCH), {}, UNSUPPORTED),
    "unknown_mode": (dict(mode=2), {}, UNSUPPORTED),
    "cosine_not_0_or_1": (dict(cosine=2), {}, UNSUPPORTED),
    "u_stride_odd": ({}, dict(u_stride=9), UNSUPPORTED),
    "v_stride_short": ({}, dict(v_stride=4), UNSUPPORTED),
    "u_null": ({}, dict(u=0), INVALID),
    "v_misaligned": ({}, dict(v="+4"), INVALID),
    "lse_null": ({}, dict(lse=0), INVALID),
    "rmax_null": ({}, dict(rmax=0), INVALID),
    "ru_null_with_cosine": ({}, dict(ru=0), INVALID),
    "w_misaligned": ({}, dict(w="+2"), INVALID),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_both_entries_refuse_and_launch_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.fwd() == code and c.bwd() == code, name
    assert c.untouched(), name


FWD_ONLY = {"loss_null": (dict(loss=0), INVALID), "rank_null": (dict(rank=0), INVALID), "sim_stride_short": (dict(sim_stride=4), UNSUPPORTED),
            "ws_null": (dict(ws=0), WORKSPACE), "ws_misaligned": (dict(ws="+16"), WORKSPACE), "ws_short": (dict(ws_bytes=4), WORKSPACE)}
BWD_ONLY = {"grad_loss_null": (dict(grad_loss=0), INVALID), "du_null": (dict(du=0), INVALID), "dv_misaligned": (dict(dv="+4"), INVALID),
            "du_stride_short": (dict(du_stride=4), UNSUPPORTED), "dv_stride_odd": (dict(dv_stride=9), UNSUPPORTED)}


@pytest.mark.parametrize("name", sorted(FWD_ONLY))
def test_the_forward_refuses(dev, name):
    fields, code = FWD_ONLY[name]
    c = Call(dev)
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.fwd() == code and c.untouched(), name


@pytest.mark.parametrize("name", sorted(BWD_ONLY))
def test_the_backward_refuses(dev, name):
    fields, code = BWD_ONLY[name]
    c = Call(dev)
    assert c.fwd() == OK
    before = {k: v.clone() for k, v in c.out.items()}
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.bwd() == code, name
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(torch.equal(before[k], c.out[k]) for k in before), name  # (du, dv still hold the sentinel)


def test_null_struct_and_workspace_query(dev):
    L = _lib.lib()
    assert L.tzr_match_softmax_fwd(None, None) == INVALID and L.tzr_match_softmax_bwd(None, None) == INVALID
    assert L.tzr_match_softmax_workspace(None) == 256
    c = Call(dev, B=33, M=40)
    assert L.tzr_match_softmax_workspace(C.byref(c.m)) == 256 + 256  # two blocks of 32 rows: four floats, rounded up, plus the slack


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    assert C.sizeof(_lib.TzrMatchSoftmax) == 224 and _lib.ABI_VERSION == 15
    assert "#define TZR_MATCH_SOFTMAX_MAX_D 256" in header and _lib.MATCH_SOFTMAX_MAX_D == 256
    assert "#define TZR_MATCH_SAMPLED 0" in header and "#define TZR_MATCH_IN_BATCH 1" in header
    assert (_lib.MATCH_SAMPLED, _lib.MATCH_IN_BATCH) == (0, 1)
    for name in ("tzr_match_softmax_workspace", "tzr_match_softmax_fwd", "tzr_match_softmax_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    fields = [n for n, _ in _lib.TzrMatchSoftmax._fields_]
    body = header[header.index("typedef struct TzrMatchSoftmax {"):header.index("} TzrMatchSoftmax;")]
    pos = [body.index(f" {n}") for n in fields if n not in ("M", "mode", "cosine", "reserved")]
    assert pos == sorted(pos)  # the same order
