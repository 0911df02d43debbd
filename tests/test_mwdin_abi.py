"""tzr_mwdin_fwd / _bwd / _workspace at the C boundary: every refusal returns its error code and launches nothing -- the outputs,
pre-filled with a sentinel, are untouched -- and the struct, the limits and the symbols agree with the header."""
import ctypes as C
import os

import pytest
import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
SENTINEL = 12345.0


class Call:
    """a valid call (lengths 2, 0, 5, C = 8, layers [8, 4] with PReLU, windows [1, 2, 3], max_len 20) whose every output holds the sentinel"""

    def __init__(self, dev, C_=8, hidden=(8, 4), windows=(1, 2, 3), max_len=20, B=3):
        f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
        lengths = [2, 0, 5][:B]
        N, Cb, W = sum(lengths), min(max(C_, 4), 128), min(max(len(windows), 1), 32)  # (buffers as large as any claim the kernel could act on)
        self.dev, self.off = dev, torch.tensor([0] + lengths, dtype=torch.int64).cumsum(0).to(dev)
        Hb = [min(max(h, 4), 128) for h in hidden[:3]]
        self.keep = [torch.randn(N, Cb).to(dev), torch.randn(max(B, 1), Cb).to(dev), torch.randn(max(B, 1), (W + 1) * Cb).to(dev),
                     torch.randn(1, Hb[-1]).to(dev), torch.randn(1).to(dev), torch.full((1,), 0.25).to(dev)]
        params = sum((d + 1) * h for d, h in zip([3 * Cb] + Hb[:-1], Hb)) + Hb[-1] + 2 + len(Hb)
        self.out = {"out": f(max(B, 1), (W + 1) * Cb), "dk": f(N, Cb), "dq": f(max(B, 1), Cb), "dparams": f(params)}
        m = self.m = _lib.TzrMwdin()
        m.B, m.N, m.C, m.W, m.max_len, m.layers = B, N, C_, len(windows), max_len, len(hidden)
        for i, w in enumerate(windows[:32]):
            m.windows_len[i] = w
        for l, (d, h) in enumerate(zip([3 * Cb] + Hb[:-1], Hb)):
            self.keep += [torch.randn(h, d).to(dev), torch.randn(h).to(dev), torch.full((1,), 0.25).to(dev)]
            m.H[l], m.w[l], m.b[l], m.slope[l] = hidden[l], *[t.data_ptr() for t in self.keep[-3:]]
        x, q, g, w3, b3, al = self.keep[:6]
        m.k, m.k_stride, m.q, m.q_stride, m.offsets = x.data_ptr(), Cb, q.data_ptr(), Cb, self.off.data_ptr()
        m.w3, m.b3, m.alpha, m.grad_out, m.grad_out_stride = w3.data_ptr(), b3.data_ptr(), al.data_ptr(), g.data_ptr(), (W + 1) * Cb
        for k in ("out", "dk", "dq", "dparams"):
            setattr(m, k, self.out[k].data_ptr())
        m.out_stride, m.dk_stride, m.dq_stride = (W + 1) * Cb, Cb, Cb
        self.ws = _lib.workspace(max(_lib.lib().tzr_mwdin_workspace(C.byref(m)), 256 + 4 * params * max(B, 1)), dev)
        m.ws, m.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def fwd(self):
        return _lib.lib().tzr_mwdin_fwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def bwd(self):
        return _lib.lib().tzr_mwdin_bwd(C.byref(self.m), _lib.stream_ptr(self.dev))

    def untouched(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.out.values())


def test_a_valid_call_writes_every_output_and_an_empty_batch_none(dev):
    c = Call(dev)
    assert c.fwd() == OK and c.bwd() == OK
    assert not any(bool((t == SENTINEL).any()) for t in c.out.values())
    c = Call(dev, B=0)
    assert c.fwd() == OK and c.bwd() == OK and c.untouched()


REFUSALS = {
    "C_not_multiple_of_4": (dict(C_=6), {}, UNSUPPORTED), "C_above_128": (dict(C_=132), {}, UNSUPPORTED), "C_below_4": (dict(C_=0), {}, UNSUPPORTED),
    "no_layer": ({}, dict(layers=0), UNSUPPORTED), "four_layers": ({}, dict(layers=4), UNSUPPORTED),
    "width_not_multiple_of_4": (dict(hidden=(8, 6)), {}, UNSUPPORTED), "width_above_128": (dict(hidden=(132,)), {}, UNSUPPORTED),
    "no_window": ({}, dict(W=0), UNSUPPORTED), "windows_above_32": ({}, dict(W=33), UNSUPPORTED), "window_of_length_0": (dict(windows=(1, 0, 3)), {}, UNSUPPORTED),
    "positions_above_128": (dict(windows=(100, 100), max_len=129), {}, UNSUPPORTED), "max_len_zero": ({}, dict(max_len=0), UNSUPPORTED),
    "tile_above_8192": (dict(C_=128, windows=(65,), max_len=65), {}, UNSUPPORTED),
    "parameters_above_the_cap": (dict(C_=128, hidden=(128, 128, 128)), {}, UNSUPPORTED),
    "k_stride_odd": ({}, dict(k_stride=9), UNSUPPORTED), "q_stride_short": ({}, dict(q_stride=4), UNSUPPORTED),
    "B_negative": ({}, dict(B=-1), INVALID), "N_negative": ({}, dict(N=-1), INVALID), "k_null": ({}, dict(k=0), INVALID),
    "k_misaligned": ({}, dict(k="+4"), INVALID), "offsets_null": ({}, dict(offsets=0), INVALID), "w3_null": ({}, dict(w3=0), INVALID),
    "alpha_null": ({}, dict(alpha=0), INVALID),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_both_entries_refuse_and_launch_nothing(dev, name):
    shape, fields, code = REFUSALS[name]
    c = Call(dev, **shape)
    for k, v in fields.items():
        setattr(c.m, k, getattr(c.m, k) + int(v) if isinstance(v, str) else v)
    assert c.fwd() == code and c.bwd() == code and c.untouched(), name


@pytest.mark.parametrize("fields,code", [(dict(ws=0), WORKSPACE), (dict(ws_bytes=4), WORKSPACE), (dict(dk_stride=9), UNSUPPORTED), (dict(dparams=0), INVALID)])
def test_the_backward_refuses(dev, fields, code):
    c = Call(dev)
    for k, v in fields.items():
        setattr(c.m, k, v)
    assert c.bwd() == code and c.untouched()


@pytest.mark.parametrize("shape", [dict(C_=96, hidden=(36,)), dict(C_=64, hidden=(64, 32)), dict(C_=128, hidden=(64,), windows=(64,), max_len=64), dict(C_=4, hidden=(4,), windows=(1,), max_len=1)])
def test_the_limits_themselves_are_taken(dev, shape):
    c = Call(dev, **shape)
    assert c.fwd() == OK and c.bwd() == OK


def test_no_rows_still_write_the_output_rows(dev):
    c = Call(dev, B=2)
    c.off.zero_()
    c.m.N, c.m.k, c.m.dk = 0, 0, 0
    assert c.fwd() == OK and c.bwd() == OK
    out, q = c.out["out"][:2], c.keep[1][:2]
    assert float(out[:, :24].abs().sum()) == 0.0 and torch.equal(out[:, 24:], q) and torch.equal(c.out["dq"][:2], c.keep[2][:2, 24:])


def test_rows_outside_the_offsets_get_zero_gradient_rows(dev):
    c = Call(dev)
    c.off.copy_(torch.tensor([1, 2, 2, 6]))  # rows 0 and 6 of the 7 belong to no sample
    assert c.fwd() == OK and c.bwd() == OK
    dk = c.out["dk"]
    assert float(dk[0].abs().sum()) == 0.0 and float(dk[6].abs().sum()) == 0.0 and not bool((dk == SENTINEL).any()) and float(dk[1:6].abs().sum()) > 0.0


def test_a_relu_layer_has_a_zero_slope_gradient(dev):
    """dparams ends [.., slope gradient of layer 0, of layer 1, dalpha]; a null slope pointer is ReLU: slope 0, gradient slot 0"""
    c = Call(dev)
    c.m.slope[1] = 0
    assert c.fwd() == OK and c.bwd() == OK
    assert float(c.out["dparams"][-2]) == 0.0 and float(c.out["dparams"][-3]) != 0.0


def test_struct_limits_and_symbols_match_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    L = _lib.lib()
    assert C.sizeof(_lib.TzrMwdin) == 400 and _lib.ABI_VERSION == 15 and L.tzr_mwdin_fwd(None, None) == INVALID and L.tzr_mwdin_workspace(None) == 256
    for name, value in (("MAX_DIM", 128), ("MAX_LAYERS", 3), ("MAX_WINDOWS", 32), ("MAX_S", 128), ("MAX_SH", 8192), ("MAX_PARAMS", 32768), ("BWD_MAX_GRID", 512)):
        assert f"#define TZR_MWDIN_{name} {value}\n" in header and getattr(_lib, f"MWDIN_{name}") == value
    for name in ("tzr_mwdin_workspace", "tzr_mwdin_fwd", "tzr_mwdin_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
