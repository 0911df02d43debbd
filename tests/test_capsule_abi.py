"""tzr_capsule_fwd / _bwd / _workspace at the C boundary: every refusal returns its error code and launches nothing -- the
outputs, pre-filled with a sentinel, are untouched -- and the struct, the limits and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
SENTINEL = 12345.0


class Call:
    """a valid call (B = 3, lengths 2, 0, 5, L = 8, H = 8, K = 4, S = 20) whose every output holds the sentinel"""

    def __init__(self, dev, L=8, H=8, K=4, S=20, iters=3, B=3):
        f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
        lengths = [2, 0, 5][:B] + [1] * max(B - 3, 0)
        N = sum(lengths)
        self.dev = dev
        self.off = torch.tensor([0] + lengths, dtype=torch.int64).cumsum(0).to(dev)
        Lb, Hb, Kb = max(L, 4), max(H, 4), max(K, 1)  # (buffers as large as the largest claim made of them)
        self.x, self.w, self.l0 = torch.randn(N, Lb).to(dev), torch.randn(Lb, Hb).to(dev), torch.randn(N, Kb).to(dev)
        self.g = torch.randn(max(B, 1) * Kb, Hb).to(dev)
        self.out = {"high": f(max(B, 1) * Kb, Hb), "pre": f(max(B, 1), Kb, Hb), "c": f(N, Kb), "dx": f(N, Lb), "dw": f(Lb, Hb),
                    "mask": torch.full((max(B, 1), Kb), 77, dtype=torch.uint8, device=dev)}
        m = self.m = _lib.TzrCapsule()
        m.B, m.N, m.L, m.H, m.K, m.S, m.num_iters, m.const_caps_num = B, N, L, H, K, S, iters, 0
        m.scale, m.stddev, m.squash_pow = 20.0, 1.0, 1.0
        m.x, m.x_stride, m.offsets, m.w, m.logits0 = self.x.data_ptr(), Lb, self.off.data_ptr(), self.w.data_ptr(), self.l0.data_ptr()
        for k in ("high", "pre", "c", "dx", "dw", "mask"):
            setattr(m, k, self.out[k].data_ptr())
        m.high_stride, m.dx_stride, m.grad_high, m.grad_high_stride = Hb, Lb, self.g.data_ptr(), Hb
        self.ws = _lib.workspace(max(_lib.lib().tzr_capsule_workspace(C.byref(m)), 256 + 4 * Lb * Hb * max(B, 1)), dev)
        m.ws, m.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def fwd(self):
        return _lib.lib().tzr_capsule_fwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def bwd(self):
        return _lib.lib().tzr_capsule_bwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def untouched(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return all(bool((t == (77 if t.dtype == torch.uint8 else SENTINEL)).all()) for t in self.out.values())


def apply(c, fields):
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)


def test_a_valid_call_runs_and_writes(dev):
    c = Call(dev)
    assert c.fwd() == OK and c.bwd() == OK
    for k in ("high", "pre", "c", "dx", "dw", "mask"):
        assert not bool((c.out[k] == (77 if k == "mask" else SENTINEL)).any()), k
    assert c.out["mask"].cpu().tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 0]]  # lengths 2, 0, 5


def test_an_empty_batch_is_ok_and_launches_nothing(dev):
    c = Call(dev, B=0)
    assert c.fwd() == OK and c.bwd() == OK and c.untouched()


REFUSALS = {
    "L_not_multiple_of_4": (dict(L=6), {}, UNSUPPORTED),
    "L_below_4": (dict(L=0), {}, UNSUPPORTED),
    "L_above_128": (dict(L=132), {}, UNSUPPORTED),
    "H_not_multiple_of_4": (dict(H=6), {}, UNSUPPORTED),
    "H_below_4": (dict(H=0), {}, UNSUPPORTED),
    "H_above_128": (dict(H=132), {}, UNSUPPORTED),
    "K_zero": (dict(K=0), {}, UNSUPPORTED),
    "K_above_8": (dict(K=9), {}, UNSUPPORTED),
    "iters_zero": (dict(iters=0), {}, UNSUPPORTED),
    "iters_above_8": (dict(iters=9), {}, UNSUPPORTED),
    "S_zero": (dict(S=0), {}, UNSUPPORTED),
    "S_above_128": (dict(S=129), {}, UNSUPPORTED),
    "S_above_128_at_H_64": (dict(S=129, H=64), {}, UNSUPPORTED),
    "S_above_64_at_H_128": (dict(S=65, H=128), {}, UNSUPPORTED),
    "SH_above_8192": (dict(S=128, H=68), {}, UNSUPPORTED),
    "scale_zero": ({}, dict(scale=0.0), UNSUPPORTED),
    "const_caps_num_not_0_or_1": ({}, dict(const_caps_num=2), UNSUPPORTED),
    "x_stride_odd": ({}, dict(x_stride=9), UNSUPPORTED),
    "x_stride_short": ({}, dict(x_stride=4), UNSUPPORTED),
    "B_negative": ({}, dict(B=-1), INVALID),
    "N_negative": ({}, dict(N=-1), INVALID),
    "x_null": ({}, dict(x=0), INVALID),
    "x_misaligned": ({}, dict(x="+4"), INVALID),
    "offsets_null": ({}, dict(offsets=0), INVALID),
    "offsets_misaligned": ({}, dict(offsets="+4"), INVALID),
    "w_null": ({}, dict(w=0), INVALID),
    "w_misaligned": ({}, dict(w="+4"), INVALID),
    "logits0_misaligned": ({}, dict(logits0="+2"), INVALID),
    "c_null": ({}, dict(c=0), INVALID),
    "pre_null": ({}, dict(pre=0), INVALID),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_both_entries_refuse_and_launch_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    apply(c, fields)
    assert c.fwd() == code and c.bwd() == code, name
    assert c.untouched(), name


@pytest.mark.parametrize("shape", [dict(L=128, H=128, S=64), dict(H=64, S=128), dict(K=8, iters=8), dict(L=4, H=4, K=1, S=1, iters=1)])
def test_the_limits_themselves_are_taken(dev, shape):
    c = Call(dev, **shape)
    assert c.fwd() == OK and c.bwd() == OK


FWD_ONLY = {"high_null": (dict(high=0), INVALID), "high_misaligned": (dict(high="+4"), INVALID), "high_stride_short": (dict(high_stride=4), UNSUPPORTED),
            "high_stride_odd": (dict(high_stride=9), UNSUPPORTED), "mask_null": (dict(mask=0), INVALID)}
BWD_ONLY = {"grad_high_null": (dict(grad_high=0), INVALID), "grad_high_misaligned": (dict(grad_high="+4"), INVALID),
            "grad_high_stride_short": (dict(grad_high_stride=4), UNSUPPORTED), "dx_null": (dict(dx=0), INVALID),
            "dx_misaligned": (dict(dx="+4"), INVALID), "dx_stride_odd": (dict(dx_stride=9), UNSUPPORTED), "dw_null": (dict(dw=0), INVALID),
            "ws_null": (dict(ws=0), WORKSPACE), "ws_misaligned": (dict(ws="+16"), WORKSPACE), "ws_short": (dict(ws_bytes=4), WORKSPACE)}


@pytest.mark.parametrize("name", sorted(FWD_ONLY))
def test_the_forward_refuses(dev, name):
    fields, code = FWD_ONLY[name]
    c = Call(dev)
    apply(c, fields)
    assert c.fwd() == code and c.untouched(), name


@pytest.mark.parametrize("name", sorted(BWD_ONLY))
def test_the_backward_refuses(dev, name):
    fields, code = BWD_ONLY[name]
    c = Call(dev)
    assert c.fwd() == OK
    before = {k: v.clone() for k, v in c.out.items()}
    apply(c, fields)
    assert c.bwd() == code, name
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(torch.equal(before[k], c.out[k]) for k in before), name  # (dx, dw still hold the sentinel)


def test_no_rows_need_no_row_pointers(dev):
    """N == 0: x, c, logits0 and dx may be null; every sample is empty, high is zeros with one valid capsule"""
    c = Call(dev, B=2)
    c.off.zero_()
    c.m.N, c.m.x, c.m.c, c.m.logits0, c.m.dx = 0, 0, 0, 0, 0
    assert c.fwd() == OK and c.bwd() == OK
    assert float(c.out["high"][:8].abs().sum()) == 0.0 and c.out["mask"].cpu().tolist() == [[1, 0, 0, 0], [1, 0, 0, 0]]
    assert float(c.out["dw"].abs().sum()) == 0.0


def test_null_struct_and_workspace_query(dev):
    L = _lib.lib()
    assert L.tzr_capsule_fwd(None, None) == INVALID and L.tzr_capsule_bwd(None, None) == INVALID
    assert L.tzr_capsule_workspace(None) == 256
    c = Call(dev)
    assert L.tzr_capsule_workspace(C.byref(c.m)) == 3 * 8 * 8 * 4 + 256  # one [L x H] row a workgroup, one workgroup a sample
    c.m.B = _lib.CAPSULE_BWD_MAX_GRID + 5
    assert L.tzr_capsule_workspace(C.byref(c.m)) == _lib.CAPSULE_BWD_MAX_GRID * 8 * 8 * 4 + 256  # (the grid is capped)


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    assert C.sizeof(_lib.TzrCapsule) == 192 and _lib.ABI_VERSION == 15
    for name, value in (("MAX_DIM", 128), ("MAX_K", 8), ("MAX_ITERS", 8), ("MAX_S", 128), ("MAX_SH", 8192), ("BWD_MAX_GRID", 512)):
        assert f"#define TZR_CAPSULE_{name} {value}\n" in header and getattr(_lib, f"CAPSULE_{name}") == value
    for name in ("tzr_capsule_workspace", "tzr_capsule_fwd", "tzr_capsule_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    fields = [n for n, _ in _lib.TzrCapsule._fields_]
    body = header[header.index("typedef struct TzrCapsule {"):header.index("} TzrCapsule;")]
    pos = [body.index(f" {n};") for n in fields if n not in ("B", "N", "L", "H", "K", "S", "num_iters", "const_caps_num", "scale", "stddev", "squash_pow", "reserved")]
    assert pos == sorted(pos)  # the same order
