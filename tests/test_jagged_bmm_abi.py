"""tzr_jagged_bmm_fwd / _bwd at the C boundary: a valid call overwrites every output, every refusal returns its error code and launches
nothing -- the outputs, pre-filled with a sentinel, are untouched -- offsets of any value stay inside the buffers, and the struct, the
limits and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -4
SENTINEL = 12288.0
DIM = _lib.JAGGED_BMM_MAX_DIM


class Call:
    """a valid call (lengths 5, 0, 70 behind two spare rows, one behind; K = 8 and N = 12 in rows 8 wider) whose outputs hold the sentinel"""

    def __init__(self, dev, K=8, N=12, offsets=(2, 7, 7, 77)):
        Kw, Nw = min(max(K, 4), DIM) + 8, min(max(N, 4), DIM) + 8  # (buffers as large as any claim the kernel could act on)
        full = lambda *s: torch.full(s, SENTINEL, device=dev)  # noqa: E731
        self.dev, self.off = dev, torch.tensor(offsets, dtype=torch.int64).to(dev)
        self.ins = [torch.randn(*s).to(dev) for s in ((78, Kw), (3, Kw - 8, Nw - 8), (3, Nw - 8), (78, Nw))]  # jagged, dense, bias, grad_out
        self.outs = {"out": full(78, Nw), "d_jagged": full(78, Kw), "d_dense": full(3, Kw, Nw), "d_bias": full(3, Nw)}
        m = self.m = _lib.TzrJaggedBmm()
        m.L, m.B, m.K, m.N, m.max_seq_len, m.offsets = 78, 3, K, N, 40, self.off.data_ptr()
        (m.jagged, m.dense, m.bias, m.grad_out), m.jagged_stride, m.grad_out_stride = (t.data_ptr() for t in self.ins), Kw, Nw
        for name, t in self.outs.items():
            setattr(m, name, t.data_ptr())
        m.out_stride, m.d_jagged_stride = Nw, Kw

    def go(self, entry):
        rc = getattr(_lib.lib(), entry)(C.byref(self.m), _lib.stream_ptr(self.dev))
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t in self.outs.values())


def test_a_valid_call_writes_every_output_and_an_empty_one_nothing(dev):
    c = Call(dev)
    assert c.go("tzr_jagged_bmm_fwd") == OK and c.go("tzr_jagged_bmm_bwd") == OK
    for name, w in (("out", 12), ("d_jagged", 8)):
        t = c.outs[name]
        assert not bool((t[:, :w] == SENTINEL).any()) and bool((t[:, w:] == SENTINEL).all())  # (the buffer's spare columns stay)
        assert not t[[0, 1, 77], :w].any() and not t[7 + 40:77, :w].any() and bool(t[[2, 6, 7, 46], :w].any(dim=1).all())
    dd, db = c.outs["d_dense"].view(-1), c.outs["d_bias"].view(-1)  # (contiguous [3, 8, 12] and [3, 12]: the head of the wider buffers)
    assert not bool((dd[:288] == SENTINEL).any()) and bool((dd[288:] == SENTINEL).all()) and not bool((db[:36] == SENTINEL).any())
    assert not dd[96:192].any() and not db[12:24].any() and bool((db[36:] == SENTINEL).all())  # the empty sample: zeros
    want = c.ins[3][7:47, :12].double().sum(0)
    assert float((db[24:36].double() - want).abs().max()) <= 2.0 ** -20 * 40  # (forty O(1) rows added in fp32)
    for field in ("L", "B"):
        c = Call(dev)
        setattr(c.m, field, 0)
        c.m.jagged = c.m.dense = c.m.offsets = 0  # (whatever the pointers are)
        assert c.go("tzr_jagged_bmm_fwd") == OK and c.go("tzr_jagged_bmm_bwd") == OK and c.untouched()


REFUSALS = {
    "K_not_multiple_of_4": (dict(K=6), {}, INVALID), "K_above_the_limit": (dict(K=DIM + 4), {}, INVALID), "K_zero": (dict(K=0), {}, INVALID),
    "N_not_multiple_of_4": (dict(N=10), {}, INVALID), "N_above_the_limit": (dict(N=DIM + 4), {}, INVALID), "N_negative": (dict(N=-4), {}, INVALID),
    "L_negative": ({}, dict(L=-1), INVALID), "B_negative": ({}, dict(B=-1), INVALID), "jagged_null": ({}, dict(jagged=0), INVALID),
    "dense_null": ({}, dict(dense=0), INVALID), "dense_misaligned": ({}, dict(dense="+4"), INVALID), "offsets_null": ({}, dict(offsets=0), INVALID),
    "bias_null": ({}, dict(bias=0, d_bias=0), INVALID), "outputs_null": ({}, dict(out=0, d_jagged=0), INVALID),
    "outputs_misaligned": ({}, dict(out="+4", d_dense="+4"), INVALID), "grad_out_null": ({}, dict(out=0, grad_out=0), INVALID),
    "max_seq_len_zero": ({}, dict(max_seq_len=0), UNSUPPORTED), "max_seq_len_above_the_limit": ({}, dict(max_seq_len=_lib.HSTU_MAX_SEQ_LEN + 1), UNSUPPORTED),
    "L_above_the_limit": ({}, dict(L=2 ** 31), UNSUPPORTED), "stride_odd": ({}, dict(jagged_stride=17), UNSUPPORTED),
    "stride_short": ({}, dict(out_stride=8, grad_out_stride=8), UNSUPPORTED),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_the_entries_refuse_and_launch_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.go("tzr_jagged_bmm_fwd") == code and c.go("tzr_jagged_bmm_bwd") == code and c.untouched(), name


@pytest.mark.parametrize("offsets", [(-5, -1, 3, 9), (60, 40, 20, 0), (0, 2 ** 40, -2 ** 40, 90), (78, 78, 78, 78)])
def test_offsets_of_any_value_stay_inside_the_buffers(dev, offsets):
    c = Call(dev, offsets=offsets)
    guard = [t[:, -8:].clone() for t in (c.outs["out"], c.outs["d_jagged"])]
    assert c.go("tzr_jagged_bmm_fwd") == OK and c.go("tzr_jagged_bmm_bwd") == OK
    assert all(torch.equal(t[:, -8:], g) for t, g in zip((c.outs["out"], c.outs["d_jagged"]), guard))
    assert all(bool(torch.isfinite(t).all()) for t in c.outs.values())


@pytest.mark.parametrize("shape", [dict(K=DIM, N=4), dict(K=4, N=DIM)])
def test_the_limits_themselves_are_taken(dev, shape):
    c = Call(dev, **shape)
    assert c.go("tzr_jagged_bmm_fwd") == OK and c.go("tzr_jagged_bmm_bwd") == OK


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    L = _lib.lib()
    assert C.sizeof(_lib.TzrJaggedBmm) == 136 and L.tzr_jagged_bmm_fwd(None, None) == INVALID and L.tzr_jagged_bmm_bwd(None, None) == INVALID
    for name, v in (("MAX_DIM", DIM), ("BLOCK", _lib.JAGGED_BMM_BLOCK), ("CHUNK", _lib.JAGGED_BMM_CHUNK)):
        assert f"#define TZR_JAGGED_BMM_{name} {v}\n" in header
    for name in ("tzr_jagged_bmm_fwd", "tzr_jagged_bmm_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
