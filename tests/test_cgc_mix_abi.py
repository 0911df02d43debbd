"""Error behaviour of tzr_cgc_mix_fwd / tzr_cgc_mix_bwd (csrc/gate_mix.hip), as tests/test_cross_v2_abi.py checks the cross
network's entry points: bad arguments come back as negative status codes -- never a crash, never a launch -- and B == 0 is a
TZR_OK no-op that reads and writes nothing."""
import ctypes as C
import os

import torch

from torcheasyrec_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -4
B, H, E = 5, 8, 4
SELS = [[0, 3], [1, 2, 3], [0, 1, 2, 3]]
SENTINEL = 7.0


def test_cgc_mix_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    G = len(SELS)
    experts = [torch.ones(B, H + 4, dtype=torch.float32, device=dev) for _ in range(E)]
    gouts = [torch.ones(B, H + 4, dtype=torch.float32, device=dev) for _ in range(G)]
    logits = [torch.zeros(B, len(s) + 1, dtype=torch.float32, device=dev) for s in SELS]
    outs = [torch.full((B, H + 4), SENTINEL, dtype=torch.float32, device=dev) for _ in range(G)]
    probs = [torch.full((B, len(s)), SENTINEL, dtype=torch.float32, device=dev) for s in SELS]
    dx = [torch.full((B, H + 4), SENTINEL, dtype=torch.float32, device=dev) for _ in range(E)]
    dl = [torch.full((B, len(s) + 1), SENTINEL, dtype=torch.float32, device=dev) for s in SELS]
    written = outs + probs + dx + dl

    def good():
        m = _lib.TzrCgcMix()
        m.B, m.H, m.n_experts, m.n_gates = B, H, E, G
        for e in range(E):
            m.expert[e], m.expert_stride[e] = p(experts[e]), H + 4
            m.d_expert[e], m.d_expert_stride[e] = p(dx[e]), H + 4
        for g, sel in enumerate(SELS):
            m.n_sel[g] = len(sel)
            for j, e in enumerate(sel):
                m.sel[g][j] = e
            m.logits[g], m.logits_stride[g] = p(logits[g]), len(sel) + 1
            m.probs[g] = p(probs[g])
            m.out[g], m.out_stride[g] = p(outs[g]), H + 4
            m.grad_out[g], m.grad_out_stride[g] = p(gouts[g]), H + 4
            m.d_logits[g], m.d_logits_stride[g] = p(dl[g]), len(sel) + 1
        return m

    def call(fn, change=None):
        m = good()
        if change is not None:
            change(m)
        return fn(C.byref(m), None)

    def setter(field, value, index=None):
        def f(m):
            if index is None:
                setattr(m, field, value)
            else:
                getattr(m, field)[index] = value
        return f

    def untouched():
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return all(float((t - SENTINEL).abs().max()) == 0.0 for t in written)

    fwd, bwd = lib.tzr_cgc_mix_fwd, lib.tzr_cgc_mix_bwd
    both = ("expert", "probs")
    for fn, arrays in ((fwd, both + ("logits", "out")), (bwd, both + ("d_expert", "grad_out", "d_logits"))):
        assert fn(None, None) == INVALID  # no struct
        for name in arrays:
            last = (E if name in ("expert", "d_expert") else G) - 1
            for i in (0, last):
                assert call(fn, setter(name, 0, i)) == INVALID, (name, i)  # a null pointer
        for name in ("expert", "d_expert", "out", "grad_out"):
            if name in arrays:
                base = {"expert": experts, "d_expert": dx, "out": outs, "grad_out": gouts}[name][1]
                assert call(fn, setter(name, p(base) + 4, 1)) == INVALID, name  # [B, H] rows that are not 16-byte aligned
                assert call(fn, setter(name, p(base) + 2, 1)) == INVALID, name
                assert call(fn, setter(name + "_stride", H + 2, 1)) == UNSUPPORTED, name  # a row stride that is no multiple of 4
                assert call(fn, setter(name + "_stride", H - 4, 1)) == UNSUPPORTED, name  # ... below H
        for name, base in (("logits", logits), ("d_logits", dl)):
            if name in arrays:
                assert call(fn, setter(name, p(base[1]) + 2, 1)) == INVALID, name  # not a float's address
                assert call(fn, setter(name + "_stride", len(SELS[1]) - 1, 1)) == UNSUPPORTED, name  # a stride below n_sel
        assert call(fn, setter("probs", p(probs[1]) + 2, 1)) == INVALID
        # sizes
        assert call(fn, setter("B", -1)) == INVALID
        for name in ("H", "n_experts", "n_gates"):
            assert call(fn, setter(name, 0)) == INVALID and call(fn, setter(name, -2)) == INVALID, name
        assert call(fn, setter("n_sel", 0, 1)) == INVALID and call(fn, setter("n_sel", -1, 2)) == INVALID
        # member lists: out of range, negative, twice in one gate
        assert call(fn, setter("sel", (C.c_int32 * 16)(0, E), 0)) == INVALID
        assert call(fn, setter("sel", (C.c_int32 * 16)(-1, 3), 0)) == INVALID
        assert call(fn, setter("sel", (C.c_int32 * 16)(1, 2, 1), 1)) == INVALID
        assert call(fn, setter("n_sel", E + 1, 2)) == INVALID  # (five members of four experts: one of them twice, or out of range)
        # limits
        assert call(fn, setter("H", 6)) == UNSUPPORTED and call(fn, setter("H", 4100)) == UNSUPPORTED
        assert call(fn, setter("n_experts", 17)) == UNSUPPORTED and call(fn, setter("n_gates", 6)) == UNSUPPORTED
        assert call(fn, setter("n_sel", 17, 1)) == UNSUPPORTED
        # no sample: nothing is launched, nothing is read or written, whatever else the struct holds
        assert call(fn, setter("B", 0)) == OK
        empty = _lib.TzrCgcMix()
        assert fn(C.byref(empty), None) == OK
    assert untouched()  # none of the calls above launched anything
    # the good calls write
    assert call(fwd) == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(float((t[:, :H] - SENTINEL).abs().min()) > 0.0 for t in outs) and all(float((t[:, H:] - SENTINEL).abs().max()) == 0.0 for t in outs)
    for g, sel in enumerate(SELS):  # equal logits: every member 1 / n_sel, every mixed value 1
        torch.testing.assert_close(probs[g].cpu(), torch.full((B, len(sel)), 1.0 / len(sel)))
        torch.testing.assert_close(outs[g][:, :H].cpu(), torch.ones(B, H))
    assert all(float((t - SENTINEL).abs().max()) == 0.0 for t in dx + dl)  # (the forward leaves the backward's outputs alone)
    assert call(bwd) == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    counts = [sum(1.0 / len(sel) for sel in SELS if e in sel) for e in range(E)]
    for e in range(E):  # grad_out = 1 everywhere: d_expert_e = the sum of its probabilities
        torch.testing.assert_close(dx[e][:, :H].cpu(), torch.full((B, H), counts[e]))
        assert float((dx[e][:, H:] - SENTINEL).abs().max()) == 0.0
    for g, sel in enumerate(SELS):  # equal dot products: the softmax backward cancels
        torch.testing.assert_close(dl[g][:, :len(sel)].cpu(), torch.zeros(B, len(sel)))
        assert float((dl[g][:, len(sel):] - SENTINEL).abs().max()) == 0.0
    # contiguous operands, the limits themselves
    assert call(fwd, setter("n_gates", 1)) == OK and call(bwd, setter("n_gates", 1)) == OK


def test_cgc_mix_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_cgc_mix_fwd", "tzr_cgc_mix_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert "typedef struct TzrCgcMix {" in header and C.sizeof(_lib.TzrCgcMix) == 1248
    assert _lib.ABI_VERSION == 15
