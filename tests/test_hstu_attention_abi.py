"""tzr_hstu_attn_fwd / _bwd at the C boundary: a valid call overwrites every output, every refusal returns its error code and
launches nothing -- the outputs, pre-filled with a sentinel, are untouched -- and the struct, the limits and the symbols agree
with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -4
SENTINEL = 12345.0


class Call:
    """a valid call (lengths 5, 0, 70 of max_seq_len 40: rows behind it; 2 rows in front of offsets[0], 1 behind offsets[B]; H = 2,
    Da = 8, Dv = 12, targets, a contextual prefix, a window) whose every output holds the sentinel"""

    def __init__(self, dev, H=2, Da=8, Dv=12, B=3):
        f = lambda d: torch.full((N, Hb, d), SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
        off = [2, 7, 7, 77][:B + 1]
        N, Hb, A, V = 78, max(H, 1), min(max(Da, 4), 128) + 4, min(max(Dv, 4), 128) + 4  # (buffers as large as any claim the kernel could act on)
        self.dev, self.off, self.nt = dev, torch.tensor(off, dtype=torch.int64).to(dev), torch.tensor([1, 0, 3], dtype=torch.int64).to(dev)
        self.keep = [torch.randn(N, Hb, A).to(dev), torch.randn(N, Hb, A).to(dev), torch.randn(N, Hb, V).to(dev), torch.randn(N, Hb, V).to(dev)]
        self.out = {"out": f(V), "dq": f(A), "dk": f(A), "dv": f(V)}
        m = self.m = _lib.TzrHstuAttn()
        m.B, m.N, m.H, m.Da, m.Dv, m.max_seq_len, m.max_attn_len, m.contextual_seq_len, m.scaling_seqlen, m.alpha = B, N, H, Da, Dv, 40, 9, 2, -1, 0.3
        m.offsets, m.num_targets = self.off.data_ptr(), self.nt.data_ptr()
        for name, t in (*zip(("q", "k", "v", "grad_out"), self.keep), *self.out.items()):
            setattr(m, name, t.data_ptr()), setattr(m, name + "_stride", t.stride(0)), setattr(m, name + "_head_stride", t.stride(1))

    def fwd(self):
        return _lib.lib().tzr_hstu_attn_fwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def bwd(self):
        return _lib.lib().tzr_hstu_attn_bwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def untouched(self, names=("out", "dq", "dk", "dv")):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return all(bool((self.out[k] == SENTINEL).all()) for k in names)


def test_a_valid_call_writes_every_row_and_an_empty_batch_none(dev):
    c = Call(dev)
    assert c.fwd() == OK and c.bwd() == OK
    for k, w in (("out", 12), ("dq", 8), ("dk", 8), ("dv", 12)):
        t = c.out[k]
        assert not bool((t[:, :, :w] == SENTINEL).any()) and bool((t[:, :, w:] == SENTINEL).all()), k  # (the buffer's spare columns stay)
        for rows in (slice(0, 2), slice(7 + 40, 78)):  # outside the offsets, behind max_seq_len: zeros
            assert float(t[rows, :, :w].abs().sum()) == 0.0, k
        assert float(t[7:47, :, :w].abs().sum()) > 0.0
    c = Call(dev, B=0)
    assert c.fwd() == OK and c.bwd() == OK and c.untouched()


REFUSALS = {
    "Da_not_multiple_of_4": (dict(Da=6), {}, UNSUPPORTED), "Da_above_128": (dict(Da=132), {}, UNSUPPORTED), "Da_below_4": (dict(Da=0), {}, UNSUPPORTED),
    "Dv_not_multiple_of_4": (dict(Dv=10), {}, UNSUPPORTED), "Dv_above_128": (dict(Dv=132), {}, UNSUPPORTED), "Dv_below_4": (dict(Dv=0), {}, UNSUPPORTED),
    "no_head": (dict(H=0), {}, UNSUPPORTED), "max_seq_len_zero": ({}, dict(max_seq_len=0), UNSUPPORTED),
    "max_seq_len_above_the_limit": ({}, dict(max_seq_len=_lib.HSTU_MAX_SEQ_LEN + 1), UNSUPPORTED),
    "q_stride_odd": ({}, dict(q_stride=25), UNSUPPORTED), "k_head_stride_short": ({}, dict(k_head_stride=4), UNSUPPORTED),
    "v_stride_short": ({}, dict(v_stride=16), UNSUPPORTED),
    "B_negative": ({}, dict(B=-1), INVALID), "N_negative": ({}, dict(N=-1), INVALID), "max_attn_len_negative": ({}, dict(max_attn_len=-1), INVALID),
    "contextual_seq_len_negative": ({}, dict(contextual_seq_len=-1), INVALID),
    "q_null": ({}, dict(q=0), INVALID), "k_misaligned": ({}, dict(k="+4"), INVALID), "v_null": ({}, dict(v=0), INVALID),
    "offsets_null": ({}, dict(offsets=0), INVALID), "num_targets_misaligned": ({}, dict(num_targets="+4"), INVALID),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_both_entries_refuse_and_launch_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.fwd() == code and c.bwd() == code and c.untouched(), name


@pytest.mark.parametrize("fields,code", [(dict(grad_out=0), INVALID), (dict(dq=0), INVALID), (dict(dk_stride=25), UNSUPPORTED), (dict(dv_head_stride=8), UNSUPPORTED)])
def test_the_backward_refuses(dev, fields, code):
    c = Call(dev)
    for k, v in fields.items():
        setattr(c.m, k, v)
    assert c.bwd() == code and c.untouched()


def test_the_forward_refuses_its_output(dev):
    c = Call(dev)
    c.m.out = 0
    assert c.fwd() == INVALID and c.untouched()


@pytest.mark.parametrize("shape", [dict(Da=128, Dv=4), dict(Da=4, Dv=128), dict(H=1, Da=4, Dv=4)])
def test_the_limits_themselves_are_taken(dev, shape):
    c = Call(dev, **shape)
    assert c.fwd() == OK and c.bwd() == OK


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    L = _lib.lib()
    assert C.sizeof(_lib.TzrHstuAttn) == 264 and _lib.ABI_VERSION == 15 and L.tzr_hstu_attn_fwd(None, None) == INVALID and L.tzr_hstu_attn_bwd(None, None) == INVALID
    for name, value in (("MAX_DIM", 128), ("MAX_SEQ_LEN", 268435456), ("BLOCK", 64), ("TILE", 16)):
        assert f"#define TZR_HSTU_{name} {value}\n" in header and getattr(_lib, f"HSTU_{name}") == value
    for name in ("tzr_hstu_attn_fwd", "tzr_hstu_attn_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
