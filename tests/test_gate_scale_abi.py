"""Error behaviour of tzr_gate_scale_fwd / tzr_gate_scale_bwd (csrc/gate_scale.hip), as tests/test_cgc_mix_abi.py checks the CGC
step's entry points: bad arguments come back as negative status codes -- never a crash, never a launch."""
import ctypes as C
import os

import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
B, H, N = 5, 8, 3
SENTINEL = 7.0


def test_gate_scale_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    new = lambda v, *s: torch.full(s, v, dtype=torch.float32, device=dev)  # noqa: E731
    zs, gouts = ([new(1.0, B, H + 4) for _ in range(N)] for _ in range(2))
    gs = [new(0.0, B, H + 4) for _ in range(N)]
    bzs, bgs = [new(0.5, H) for _ in range(N)], [new(0.0, H) for _ in range(N)]
    outs, dz, dg = ([new(SENTINEL, B, H + 4) for _ in range(N)] for _ in range(3))
    db = new(SENTINEL, N, 2, H)
    ws = _lib.workspace(lib.tzr_gate_scale_bwd_workspace(B, H, N), dev)
    written = outs + dz + dg + [db]

    def good():
        m = _lib.TzrGateScale()
        m.B, m.H, m.n_slots, m.relu, m.gamma = B, H, N, 1, 2.0
        for n in range(N):
            m.z[n], m.z_stride[n], m.g[n], m.g_stride[n] = p(zs[n]), H + 4, p(gs[n]), H + 4
            m.bz[n], m.bg[n] = p(bzs[n]), p(bgs[n])
            m.out[n], m.out_stride[n] = p(outs[n]), H + 4
            m.grad_out[n], m.grad_out_stride[n] = p(gouts[n]), H + 4
            m.dz[n], m.dz_stride[n], m.dg[n], m.dg_stride[n] = p(dz[n]), H + 4, p(dg[n]), H + 4
        m.d_bias, m.ws, m.ws_bytes = p(db), p(ws), ws.numel()
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

    fwd, bwd = lib.tzr_gate_scale_fwd, lib.tzr_gate_scale_bwd
    bases = {"z": zs, "g": gs, "out": outs, "grad_out": gouts, "dz": dz, "dg": dg}
    for fn, rows in ((fwd, ("z", "g", "out")), (bwd, ("z", "g", "grad_out", "dz", "dg"))):
        assert fn(None, None) == INVALID  # no struct
        for name in rows:
            for i in (0, N - 1):
                if name != "grad_out":  # (a null grad_out is a slot without an output gradient)
                    assert call(fn, setter(name, 0, i)) == INVALID, (name, i)  # a null row pointer
            assert call(fn, setter(name, p(bases[name][1]) + 4, 1)) == INVALID, name  # rows that are not 16-byte aligned
            assert call(fn, setter(name, p(bases[name][1]) + 2, 1)) == INVALID, name
            assert call(fn, setter(name + "_stride", H + 2, 1)) == UNSUPPORTED, name  # a row stride that is no multiple of 4
            assert call(fn, setter(name + "_stride", H + 1, 1)) == UNSUPPORTED, name  # ... odd
            assert call(fn, setter(name + "_stride", H - 4, 1)) == UNSUPPORTED, name  # ... below H
        assert call(fn, setter("bg", 0, 1)) == INVALID and call(fn, setter("bg", p(bgs[1]) + 4, 1)) == INVALID
        assert call(fn, setter("bz", p(bzs[1]) + 4, 1)) == INVALID
        # sizes and limits
        assert call(fn, setter("n_slots", 0)) == INVALID and call(fn, setter("n_slots", -1)) == INVALID
        assert call(fn, setter("n_slots", 9)) == UNSUPPORTED
        assert call(fn, setter("H", 6)) == UNSUPPORTED and call(fn, setter("H", 4100)) == UNSUPPORTED
        assert call(fn, setter("H", 0)) == INVALID and call(fn, setter("H", -4)) == INVALID
        assert call(fn, setter("B", 0)) == INVALID and call(fn, setter("B", -1)) == INVALID
        empty = _lib.TzrGateScale()
        assert fn(C.byref(empty), None) == INVALID
    assert call(bwd, setter("d_bias", 0)) == INVALID and call(bwd, setter("d_bias", p(db) + 4)) == INVALID
    assert call(bwd, setter("ws", 0)) == WORKSPACE and call(bwd, setter("ws", p(ws) + 16)) == WORKSPACE
    assert call(bwd, setter("ws_bytes", 64)) == WORKSPACE
    assert untouched()  # none of the calls above launched anything
    # the good calls write: z + bz = 1.5, g + bg = 0 -> out = 1.5 * 2 * 0.5
    assert call(fwd) == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for t in outs:
        torch.testing.assert_close(t[:, :H].cpu(), torch.full((B, H), 1.5))
        assert float((t[:, H:] - SENTINEL).abs().max()) == 0.0
    assert all(float((t - SENTINEL).abs().max()) == 0.0 for t in dz + dg + [db])  # (the forward leaves the backward's outputs alone)
    assert call(bwd, setter("grad_out", 0, 1)) == OK  # slot 1 without an output gradient
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for n in range(N):  # grad_out = 1: dz = gamma s = 1, dg = 1.5 * 2 * 0.25
        live = 0.0 if n == 1 else 1.0
        torch.testing.assert_close(dz[n][:, :H].cpu(), torch.full((B, H), 1.0 * live))
        torch.testing.assert_close(dg[n][:, :H].cpu(), torch.full((B, H), 0.75 * live))
        assert float((dz[n][:, H:] - SENTINEL).abs().max()) == 0.0 and float((dg[n][:, H:] - SENTINEL).abs().max()) == 0.0
        torch.testing.assert_close(db[n].cpu(), torch.tensor([[B * 1.0 * live] * H, [B * 0.75 * live] * H]))
    # no bias on z (EPNet), identity, one slot, in place: dz over z and dg over g
    def epnet(m):
        m.n_slots, m.relu = 1, 0
        m.bz[0] = 0
        m.dz[0], m.dg[0] = m.z[0], m.g[0]
    assert call(fwd, epnet) == OK and call(bwd, epnet) == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    torch.testing.assert_close(outs[0][:, :H].cpu(), torch.full((B, H), 1.0))
    torch.testing.assert_close(zs[0][:, :H].cpu(), torch.full((B, H), 1.0))   # dz = gamma s
    torch.testing.assert_close(gs[0][:, :H].cpu(), torch.full((B, H), 0.5))   # dg = z gamma s (1 - s)


def test_gate_scale_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_gate_scale_fwd", "tzr_gate_scale_bwd", "tzr_gate_scale_bwd_workspace"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert "typedef struct TzrGateScale {" in header and C.sizeof(_lib.TzrGateScale) == 952
    assert _lib.ABI_VERSION == 15
