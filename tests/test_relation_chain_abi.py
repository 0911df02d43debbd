"""Error behaviour of tzr_relation_chain_fwd / _bwd / _bwd_workspace (csrc/relation_chain.hip), as tests/test_gate_scale_abi.py
checks the gate-and-scale entry points: bad arguments come back as negative status codes -- never a crash, never a launch --
and the workspace size is honoured to the byte."""
import ctypes as C
import os

import torch

from torcheasyrec_amd import _lib

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
B, HX, N0, N1 = 5, 8, 12, 4  # tower 0: no layers; tower 1: [x_1 | x_0] -> 12 -> 4; tower 2: [x_2 | r_1] -> 4
SENTINEL = 7.0


def test_relation_chain_rejects_bad_arguments(dev):
    lib, p = _lib.lib(), _lib.ptr
    new = lambda v, *s: torch.full(s, v, dtype=torch.float32, device=dev)  # noqa: E731
    xs = [new(1.0, B, HX + 4) for _ in range(3)]
    gr = [new(1.0, B, HX + 4), new(1.0, B, N1 + 4), new(1.0, B, N1 + 4)]
    dims = {(1, 0): (N0, 2 * HX), (1, 1): (N1, N0), (2, 0): (N1, HX + N1)}
    ws_ = {k: new(0.0, *d) for k, d in dims.items()}
    bs = {k: new(0.5, d[0]) for k, d in dims.items()}
    hs = {k: new(SENTINEL, B, d[0]) for k, d in dims.items()}
    dws = {k: new(SENTINEL, *d) for k, d in dims.items()}
    dbs = {k: new(SENTINEL, d[0]) for k, d in dims.items()}
    dxs = [new(SENTINEL, B, HX + 4) for _ in range(3)]
    written = list(hs.values()) + list(dws.values()) + list(dbs.values()) + dxs

    def base():
        m = _lib.TzrRelationChain()
        m.B, m.n_towers = B, 3
        for t in range(3):
            m.x[t], m.x_stride[t], m.x_width[t] = p(xs[t]), HX + 4, HX
            m.grad_r[t], m.grad_r_stride[t] = p(gr[t]), gr[t].stride(0)
            m.dx[t], m.dx_stride[t] = p(dxs[t]), HX + 4
        m.n_layers[1], m.n_layers[2] = 2, 1
        m.n_deps[1], m.n_deps[2] = 1, 1
        m.deps[1][0], m.deps[2][0] = 0, 1
        for (t, l), d in dims.items():
            m.width[t][l] = d[0]
            m.w[t][l], m.b[t][l], m.h[t][l] = p(ws_[(t, l)]), p(bs[(t, l)]), p(hs[(t, l)])
            m.dw[t][l], m.db[t][l] = p(dws[(t, l)]), p(dbs[(t, l)])
        return m

    need = lib.tzr_relation_chain_bwd_workspace(C.byref(base()))
    assert need == 256 + 256 * sum(-(-B * d[0] * 4 // 256) for d in dims.values())  # every dz 256-byte aligned, plus the slack
    ws = _lib.workspace(need, dev)

    def good():
        m = base()
        m.ws, m.ws_bytes = p(ws), need - 256
        return m

    def call(fn, change=None):
        m = good()
        if change is not None:
            change(m)
        return fn(C.byref(m), None)

    def setter(field, value, *index):
        def f(m):
            if not index:
                setattr(m, field, value)
                return
            a = getattr(m, field)
            for i in index[:-1]:
                a = a[i]
            a[index[-1]] = value
        return f

    def untouched():
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return all(float((t - SENTINEL).abs().max()) == 0.0 for t in written)

    fwd, bwd = lib.tzr_relation_chain_fwd, lib.tzr_relation_chain_bwd
    for fn in (fwd, bwd):
        assert fn(None, None) == INVALID  # no struct
        assert fn(C.byref(_lib.TzrRelationChain()), None) == INVALID  # an empty one
        rows = [("x", xs)] + ([("dx", dxs), ("grad_r", gr)] if fn is bwd else [])
        for name, base_t in rows:
            for t in (1, 2):
                if name != "grad_r":  # (a null grad_r is a tower without an outside gradient)
                    assert call(fn, setter(name, 0, t)) == INVALID, (name, t)
                assert call(fn, setter(name, p(base_t[t]) + 4, t)) == INVALID, (name, t)  # rows that are not 16-byte aligned
                assert call(fn, setter(name + "_stride", base_t[t].stride(0) + 2, t)) == UNSUPPORTED, (name, t)  # no multiple of 4
                assert call(fn, setter(name + "_stride", 0, t)) == UNSUPPORTED, (name, t)  # below the width
        for name, bufs in [("w", ws_), ("b", bs), ("h", hs)] + ([("dw", dws), ("db", dbs)] if fn is bwd else []):
            for (t, l) in dims:
                assert call(fn, setter(name, 0, t, l)) == INVALID, (name, t, l)
                assert call(fn, setter(name, p(bufs[(t, l)]) + 4, t, l)) == INVALID, (name, t, l)
        # sizes, limits, the graph
        assert call(fn, setter("B", 0)) == INVALID and call(fn, setter("B", -1)) == INVALID
        assert call(fn, setter("n_towers", 0)) == INVALID and call(fn, setter("n_towers", 9)) == UNSUPPORTED
        assert call(fn, setter("x_width", 0, 0)) == INVALID and call(fn, setter("x_width", 6, 0)) == UNSUPPORTED
        assert call(fn, setter("x_width", 1028, 0)) == UNSUPPORTED
        assert call(fn, setter("n_layers", -1, 1)) == INVALID and call(fn, setter("n_layers", 5, 1)) == UNSUPPORTED
        assert call(fn, setter("width", 0, 1, 0)) == INVALID and call(fn, setter("width", 6, 1, 0)) == UNSUPPORTED
        assert call(fn, setter("width", 132, 1, 0)) == UNSUPPORTED
        assert call(fn, setter("n_deps", -1, 1)) == INVALID and call(fn, setter("n_deps", 9, 1)) == UNSUPPORTED
        assert call(fn, setter("deps", 1, 1, 0)) == INVALID  # a tower naming itself
        assert call(fn, setter("deps", 2, 1, 0)) == INVALID  # ... a later one
        assert call(fn, setter("deps", -1, 2, 0)) == INVALID

        def twice(m):
            m.n_deps[2], m.deps[2][1] = 2, 1
        assert call(fn, twice) == INVALID
    assert call(bwd, setter("ws", 0)) == WORKSPACE and call(bwd, setter("ws", p(ws) + 16)) == WORKSPACE
    assert call(bwd, setter("ws_bytes", need - 256 - 1)) == WORKSPACE  # one byte short
    assert untouched()  # none of the calls above launched anything
    # the good calls write.  W = 0, b = 0.5: every h is 0.5
    assert call(fwd) == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for h in hs.values():
        torch.testing.assert_close(h.cpu(), torch.full(h.shape, 0.5))
    assert all(float((t - SENTINEL).abs().max()) == 0.0 for t in list(dws.values()) + list(dbs.values()) + dxs)
    assert call(bwd) == OK  # (exactly the size asked for, less the slack: taken)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    # grad_r = 1, W = 0: dz of the last layers is 1 and nothing flows further; db = B there, 0 in tower 1's first layer
    torch.testing.assert_close(dbs[(1, 1)].cpu(), torch.full((N1,), float(B)))
    torch.testing.assert_close(dbs[(2, 0)].cpu(), torch.full((N1,), float(B)))
    torch.testing.assert_close(dbs[(1, 0)].cpu(), torch.zeros(N0))
    torch.testing.assert_close(dws[(2, 0)].cpu(), torch.cat([torch.full((N1, HX), float(B)), torch.full((N1, N1), 0.5 * B)], dim=1))
    torch.testing.assert_close(dws[(1, 1)].cpu(), torch.full((N1, N0), 0.5 * B))
    for t in range(3):
        torch.testing.assert_close(dxs[t][:, :HX].cpu(), torch.zeros(B, HX))
        assert float((dxs[t][:, HX:] - SENTINEL).abs().max()) == 0.0  # (the columns beside the rows stay)


def test_relation_chain_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for name in ("tzr_relation_chain_fwd", "tzr_relation_chain_bwd", "tzr_relation_chain_bwd_workspace"):
        assert name in _lib.EXPORTED_SYMBOLS and f" {name}(" in header
    assert "typedef struct TzrRelationChain {" in header and C.sizeof(_lib.TzrRelationChain) == 2176
    for name, value in (("TOWERS", 8), ("LAYERS", 4), ("WIDTH", 128), ("X", 1024)):
        assert f"#define TZR_RELATION_CHAIN_MAX_{name} {value}\n" in header and getattr(_lib, f"RELATION_CHAIN_MAX_{name}") == value
    assert _lib.ABI_VERSION == 15
