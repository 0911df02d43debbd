"""tzr_hstu_delta_fwd at the C boundary: a valid call overwrites every output row, every refusal returns its error code and launches
nothing -- the output, pre-filled with a sentinel, is untouched -- and the struct, the limits and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
SENTINEL = 12345.0
CHUNK = _lib.HSTU_DELTA_CHUNK


class Call:
    """a valid two-segment call (cached lengths 5, 0, 70 with delta 3 of max_seq_len 40: the last sample is refused; H = 2, Da = 8,
    Dv = 12, targets, a contextual prefix, a window) whose output holds the sentinel"""

    def __init__(self, dev, H=2, Da=8, Dv=12, B=3, delta=3, max_seq_len=40):
        Hb, A, V, d = max(H, 1), min(max(Da, 4), 128) + 4, min(max(Dv, 4), 128) + 4, max(delta, 1)  # (buffers as large as any claim the kernel could act on)
        self.dev, self.off, self.nt = dev, torch.tensor([2, 7, 7, 77][:B + 1], dtype=torch.int64).to(dev), torch.tensor([1, 0, 3], dtype=torch.int64).to(dev)
        self.keep = [torch.randn(n, Hb, w).to(dev) for n, w in ((3 * d, A), (78, A), (78, V), (3 * d, A), (3 * d, V))]
        self.out = torch.full((3 * d, Hb, V), SENTINEL, dtype=torch.float32, device=dev)
        m = self.m = _lib.TzrHstuDelta()
        m.B, m.Nc, m.H, m.Da, m.Dv, m.delta, m.max_seq_len, m.max_attn_len, m.contextual_seq_len, m.scaling_seqlen, m.alpha = B, 78, H, Da, Dv, delta, max_seq_len, 9, 2, -1, 0.3
        m.offsets, m.num_targets = self.off.data_ptr(), self.nt.data_ptr()
        for name, t in (*zip(("delta_q", "k", "v", "k_delta", "v_delta"), self.keep), ("out", self.out)):
            setattr(m, name, t.data_ptr()), setattr(m, name + "_stride", t.stride(0)), setattr(m, name + "_head_stride", t.stride(1))
        self.ws = _lib.workspace(_lib.lib().tzr_hstu_delta_workspace(C.byref(m)), dev)
        m.ws, m.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def fwd(self):
        return _lib.lib().tzr_hstu_delta_fwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def untouched(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return bool((self.out == SENTINEL).all())


@pytest.mark.parametrize("max_seq_len", [40, CHUNK + 40])  # one chunk: the kernel stores; two: the finishing launch does
def test_a_valid_call_writes_every_row_and_an_empty_batch_none(dev, max_seq_len):
    c = Call(dev, max_seq_len=max_seq_len)
    assert c.fwd() == OK
    t = c.out
    assert not bool((t[:, :, :12] == SENTINEL).any()) and bool((t[:, :, 12:] == SENTINEL).all())  # (the buffer's spare columns stay)
    assert float(t[:6, :, :12].abs().min()) > 0.0
    assert (float(t[6:, :, :12].abs().sum()) == 0.0) == (max_seq_len == 40)  # 70 + 3 rows: refused at max_seq_len 40
    c = Call(dev, B=0)
    assert c.fwd() == OK and c.untouched()


REFUSALS = {
    "Da_not_multiple_of_4": (dict(Da=6), {}, UNSUPPORTED), "Da_above_128": (dict(Da=132), {}, UNSUPPORTED), "Dv_below_4": (dict(Dv=0), {}, UNSUPPORTED),
    "Dv_not_multiple_of_4": (dict(Dv=10), {}, UNSUPPORTED), "no_head": (dict(H=0), {}, UNSUPPORTED), "delta_zero": (dict(delta=0), {}, UNSUPPORTED),
    "max_seq_len_zero": (dict(max_seq_len=0), {}, UNSUPPORTED), "max_seq_len_above_the_limit": ({}, dict(max_seq_len=_lib.HSTU_MAX_SEQ_LEN + 1), UNSUPPORTED),
    "Nc_above_the_limit": ({}, dict(Nc=2 ** 31), UNSUPPORTED), "delta_q_stride_odd": ({}, dict(delta_q_stride=25), UNSUPPORTED),
    "k_head_stride_short": ({}, dict(k_head_stride=4), UNSUPPORTED), "v_delta_stride_short": ({}, dict(v_delta_stride=16), UNSUPPORTED),
    "out_head_stride_short": ({}, dict(out_head_stride=8), UNSUPPORTED),
    "B_negative": ({}, dict(B=-1), INVALID), "Nc_negative": ({}, dict(Nc=-1), INVALID), "max_attn_len_negative": ({}, dict(max_attn_len=-1), INVALID),
    "contextual_seq_len_negative": ({}, dict(contextual_seq_len=-1), INVALID), "delta_q_null": ({}, dict(delta_q=0), INVALID),
    "k_misaligned": ({}, dict(k="+4"), INVALID), "v_null": ({}, dict(v=0), INVALID), "k_delta_without_v_delta": ({}, dict(v_delta=0), INVALID),
    "offsets_null": ({}, dict(offsets=0), INVALID), "num_targets_misaligned": ({}, dict(num_targets="+4"), INVALID), "out_null": ({}, dict(out=0), INVALID),
    "workspace_null": (dict(max_seq_len=CHUNK + 1), dict(ws=0), WORKSPACE), "workspace_small": (dict(max_seq_len=CHUNK + 1), dict(ws_bytes=2 * 9 * 2 * 12 * 4 - 1), WORKSPACE),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_the_entry_refuses_and_launches_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.fwd() == code and c.untouched(), name


@pytest.mark.parametrize("shape", [dict(Da=128, Dv=4), dict(Da=4, Dv=128), dict(H=1, Da=4, Dv=4, delta=1)])
def test_the_limits_themselves_are_taken(dev, shape):
    assert Call(dev, **shape).fwd() == OK


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    L = _lib.lib()
    assert C.sizeof(_lib.TzrHstuDelta) == 232 and L.tzr_hstu_delta_fwd(None, None) == INVALID and L.tzr_hstu_delta_workspace(None) == 0
    assert f"#define TZR_HSTU_DELTA_CHUNK {CHUNK}\n" in header and CHUNK % (4 * _lib.HSTU_TILE) == 0
    for name in ("tzr_hstu_delta_fwd", "tzr_hstu_delta_workspace"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
