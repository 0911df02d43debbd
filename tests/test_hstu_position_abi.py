"""tzr_hstu_pos_fwd / _bwd at the C boundary: a valid call overwrites every output, every refusal returns its error code and launches
nothing -- the outputs, pre-filled with a sentinel, are untouched -- and the struct, the limits and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
SENTINEL = 12288.0  # (a bf16 value too)
SLAB = _lib.HSTU_POS_SLAB


class Call:
    """a valid timestamp-mode call (lengths 5, 0, 70 behind two spare rows, E = 8 in rows 12 wide, P = 9, T = 4, c = 2, targets)
    whose outputs hold the sentinel"""

    def __init__(self, dev, E=8, P=9, T=4, L=78, use_time=1, bf16=0, c=2):
        dt, W = torch.bfloat16 if bf16 else torch.float32, min(max(E, 8), 512) + 8  # (buffers as large as any claim the kernel could act on)
        full = lambda *s: torch.full(s, SENTINEL, dtype=dt, device=dev)  # noqa: E731
        self.dev, self.off, self.nt = dev, torch.tensor([2, 7, 7, 77], dtype=torch.int64).to(dev), torch.tensor([1, 0, 3], dtype=torch.int64).to(dev)
        self.tm = (1000 - 50 * torch.arange(78, dtype=torch.int64)).to(dev)
        self.ins = [torch.randn(n, W).to(dev, dt) for n in (78, 78, max(P, 1), max(T, 0) + 1)]  # x, grad_out, pos, ts
        self.outs = {"out": full(78, W), "dx": full(78, W), "dpos": full(max(P, 1), W), "dts": full(max(T, 0) + 1, W)}
        self.bucket = torch.full((78,), 12345, dtype=torch.int32, device=dev)
        m = self.m = _lib.TzrHstuPos()
        m.L, m.B, m.E, m.P, m.T, m.max_seq_len, m.contextual_seq_len, m.use_time, m.bf16, m.alpha, m.time_bucket_increments = L, 3, E, P, T, 40, c, use_time, bf16, 2.0, 60.0
        m.offsets, m.num_targets, m.timestamps, m.bucket = self.off.data_ptr(), self.nt.data_ptr(), self.tm.data_ptr(), self.bucket.data_ptr()
        (m.x, m.grad_out, m.pos, m.ts), m.x_stride, m.grad_out_stride = (t.data_ptr() for t in self.ins), W, W
        m.out, m.dx, m.out_stride, m.dx_stride = self.outs["out"].data_ptr(), self.outs["dx"].data_ptr(), W, W
        # (the tables' gradients are contiguous [., E]: the head of the wider buffers)
        m.dpos, m.dts = self.outs["dpos"].data_ptr(), self.outs["dts"].data_ptr()
        self.ws = _lib.workspace(_lib.lib().tzr_hstu_pos_bwd_workspace(C.byref(m)), dev)
        m.ws, m.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def go(self, entry):
        rc = getattr(_lib.lib(), entry)(C.byref(self.m), _lib.stream_ptr(self.dev))
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t in self.outs.values()) and bool((self.bucket == 12345).all())


@pytest.mark.parametrize("bf16", [0, 1])
def test_a_valid_call_writes_every_output_and_an_empty_one_the_tables_alone(dev, bf16):
    c = Call(dev, bf16=bf16)
    assert c.go("tzr_hstu_pos_fwd") == OK and c.go("tzr_hstu_pos_bwd") == OK
    for name in ("out", "dx"):
        t = c.outs[name]
        assert not bool((t[:, :8] == SENTINEL).any()) and bool((t[:, 8:] == SENTINEL).all())  # (the buffer's spare columns stay)
    assert not bool((c.outs["dpos"].view(-1)[:9 * 8] == SENTINEL).any()) and not bool((c.outs["dts"].view(-1)[:5 * 8] == SENTINEL).any())
    assert bool((c.outs["dts"].view(-1)[5 * 8:] == SENTINEL).all())
    b = c.bucket.tolist()
    assert b[:2] == [-1, -1] and b[77] == -1 and b[7 + 40:77] == [-1] * 30 and all(0 <= v <= 4 for v in b[2:7] + b[7:47])
    c = Call(dev, L=0, bf16=bf16)
    assert c.go("tzr_hstu_pos_fwd") == OK and c.untouched()
    assert c.go("tzr_hstu_pos_bwd") == OK and float(c.outs["dpos"].view(-1)[:72].float().abs().sum()) == 0.0 and bool((c.outs["dx"] == SENTINEL).all())


REFUSALS = {
    "E_not_multiple_of_4": (dict(E=6), {}, UNSUPPORTED), "E_above_the_limit": (dict(E=516), {}, UNSUPPORTED), "E_zero": (dict(E=0), {}, UNSUPPORTED),
    "bf16_E_not_multiple_of_8": (dict(E=12, bf16=1), {}, UNSUPPORTED), "P_zero": (dict(P=0), {}, UNSUPPORTED), "T_zero": (dict(T=0), {}, UNSUPPORTED),
    "T_above_the_limit": ({}, dict(T=_lib.HSTU_POS_MAX_BUCKETS + 1), UNSUPPORTED), "c_above_P": ({}, dict(contextual_seq_len=10), UNSUPPORTED),
    "max_seq_len_zero": ({}, dict(max_seq_len=0), UNSUPPORTED), "max_seq_len_above_the_limit": ({}, dict(max_seq_len=_lib.HSTU_MAX_SEQ_LEN + 1), UNSUPPORTED),
    "L_above_the_limit": ({}, dict(L=2 ** 31), UNSUPPORTED), "x_stride_odd": ({}, dict(x_stride=17, grad_out_stride=17), UNSUPPORTED),
    "out_stride_short": ({}, dict(out_stride=4, dx_stride=4), UNSUPPORTED),
    "L_negative": ({}, dict(L=-1), INVALID), "B_negative": ({}, dict(B=-1), INVALID), "c_negative": ({}, dict(contextual_seq_len=-1), INVALID),
    "increments_zero": ({}, dict(time_bucket_increments=0.0), INVALID), "time_fn_unknown": ({}, dict(time_fn=2), INVALID),
    "x_null": ({}, dict(x=0, grad_out=0), INVALID), "out_misaligned": ({}, dict(out="+4", dx="+4"), INVALID), "pos_null": ({}, dict(pos=0, dpos=0), INVALID),
    "ts_null": ({}, dict(ts=0, dts=0), INVALID), "offsets_null": ({}, dict(offsets=0), INVALID), "num_targets_misaligned": ({}, dict(num_targets="+4"), INVALID),
    "bucket_null": ({}, dict(bucket=0), INVALID),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_the_entries_refuse_and_launch_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.go("tzr_hstu_pos_fwd") == code and c.go("tzr_hstu_pos_bwd") == code and c.untouched(), name


@pytest.mark.parametrize("fields", [dict(ws=0), dict(ws="+16"), dict(ws_bytes="-1")])
def test_a_bad_workspace_refuses_the_backward(dev, fields):
    c = Call(dev)
    c.m.ws_bytes = _lib.lib().tzr_hstu_pos_bwd_workspace(C.byref(c.m))
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.go("tzr_hstu_pos_bwd") == WORKSPACE and c.untouched()


@pytest.mark.parametrize("shape", [dict(E=512), dict(E=4, P=1, T=1, c=1), dict(E=512, bf16=1), dict(use_time=0, T=0)])
def test_the_limits_themselves_are_taken(dev, shape):
    c = Call(dev, **shape)
    assert c.go("tzr_hstu_pos_fwd") == OK and c.go("tzr_hstu_pos_bwd") == OK


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    L = _lib.lib()
    assert C.sizeof(_lib.TzrHstuPos) == 216 and L.tzr_hstu_pos_fwd(None, None) == INVALID and L.tzr_hstu_pos_bwd(None, None) == INVALID
    assert L.tzr_hstu_pos_bwd_workspace(None) == 0
    for name, v in (("MAX_DIM", _lib.HSTU_POS_MAX_DIM), ("MAX_BUCKETS", _lib.HSTU_POS_MAX_BUCKETS), ("SLAB", SLAB)):
        assert f"#define TZR_HSTU_POS_{name} {v}\n" in header
    for name in ("tzr_hstu_pos_fwd", "tzr_hstu_pos_bwd", "tzr_hstu_pos_bwd_workspace"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
