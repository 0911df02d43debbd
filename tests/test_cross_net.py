"""`Cross` (torcheasyrec_amd/interaction.py) on tzr_cross_fwd / tzr_cross_bwd (csrc/cross_net.hip): against the reference's own
module (tests/golden/reference_cross_vectors.npz) and, at the kernel's edges, against the float64 restatement of the literal
loop (tests/cross_ref.py).

Bound, per tensor kind (y, gx, gw, gb): |ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the distance of the
reference's (for the edge cases: torch's literal fp32 form's) result to float64 on the same inputs -- never anything the
code under test computed.  The factor 4 is the one tests/test_losses.py uses; the closed form of the backward measured
0.5x - 1.4x of the literal form's distance on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cross_ref as ref
from torcheasyrec_amd import _lib
from torcheasyrec_amd import interaction
from torcheasyrec_amd.interaction import Cross

VEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_cross_vectors.npz"))
NPZ_CASES = {"b6_d33_l3": (6, 33, 3), "b37_d429_l3": (37, 429, 3), "b9_d64_l1": (9, 64, 1)}
# a launch holds at most 512 workgroups x 4 waves = 2048 samples at a time (CN_MAXGRID, CN_WAVES of csrc/cross_net.hip)
CONCURRENT = 512 * 4
EDGES = [(5, 1, 1), (1, 64, 3), (33, 65, 2), (70, 1024, 8), (4 * CONCURRENT + 37, 33, 2)]


def _module(dev, D, ws, bs):
    m = Cross(D, len(ws))
    with torch.no_grad():
        for i, (w, b) in enumerate(zip(ws, bs)):
            m.w[i].weight.copy_(w)
            m.b[i].copy_(b)
    return m.to(dev)


def _run_module(m, x, gy):
    for p in m.parameters():
        p.grad = None
    x = x.detach().clone().requires_grad_(True)
    y = m(x)
    y.backward(gy)
    return {"y": [y.detach()], "gx": [x.grad], "gw": [l.weight.grad for l in m.w], "gb": [p.grad for p in m.b]}


def _run_library(dev, x, ws, bs, gy):
    """the two entry points on the tensors as they lie (x and gy may be column slices of wider tensors)"""
    lib, L, (B, D) = _lib.lib(), len(ws), x.shape
    y, s, dx = (torch.empty(B, n, dtype=torch.float32, device=dev) for n in (D, L, D))
    dwb = torch.empty(2, L, D, dtype=torch.float32, device=dev)
    pw = (C.c_void_p * L)(*[_lib.ptr(w) for w in ws])
    pb = (C.c_void_p * L)(*[_lib.ptr(b) for b in bs])
    st = _lib.stream_ptr(dev)
    assert lib.tzr_cross_fwd(_lib.ptr(x), x.stride(0), pw, pb, L, B, D, _lib.ptr(y), D, _lib.ptr(s), st) == 0
    wsp = _lib.workspace(lib.tzr_cross_bwd_workspace(B, D, L), dev)
    assert lib.tzr_cross_bwd(_lib.ptr(gy), gy.stride(0), _lib.ptr(x), x.stride(0), _lib.ptr(s), pw, pb, L, B, D, _lib.ptr(dx), D,
                             _lib.ptr(dwb[0]), _lib.ptr(dwb[1]), _lib.ptr(wsp), wsp.numel(), st) == 0
    return {"y": [y], "gx": [dx], "gw": [dwb[0, l] for l in range(L)], "gb": [dwb[1, l] for l in range(L)]}


def _bit_equal(a, b):
    return all(torch.equal(p.reshape(-1), q.reshape(-1)) for k in ref.KINDS for p, q in zip(a[k], b[k]))


@pytest.mark.parametrize("tag", list(NPZ_CASES))
def test_module_matches_the_reference_module(dev, tag):
    B, D, L = NPZ_CASES[tag]
    x, gy = torch.from_numpy(VEC[f"{tag}/x"]), torch.from_numpy(VEC[f"{tag}/gy"])
    ws = [torch.from_numpy(VEC[f"{tag}/w{i}"]) for i in range(L)]
    bs = [torch.from_numpy(VEC[f"{tag}/b{i}"]) for i in range(L)]
    assert x.shape == (B, D) and all(float(b.abs().max()) > 0 for b in bs)
    want = ref.cross_literal(x, ws, bs, gy)
    gaps = {k: float(VEC[f"ref_gap/{tag}/{k}"]) for k in ref.KINDS}
    # the stored results are the reference's: the restatement reproduces them to the stored gap
    stored = {"y": [torch.from_numpy(VEC[f"{tag}/y"])], "gx": [torch.from_numpy(VEC[f"{tag}/gx"])],
              "gw": [torch.from_numpy(VEC[f"{tag}/gw{i}"]) for i in range(L)], "gb": [torch.from_numpy(VEC[f"{tag}/gb{i}"]) for i in range(L)]}
    for k in ref.KINDS:
        assert abs(ref.rel_err(stored[k], want[k]) - gaps[k]) <= 1e-12, k
    m = _module(dev, D, ws, bs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (1, 1)
    ref.check(got, want, gaps, f"{tag} on {dev.type}")
    assert got["gw"][0].shape == (1, D) and got["gb"][0].shape == (D,)


def _count_calls():
    """(forward, backward) calls of the library since this call; restored by the `dev` fixture's next use_library"""
    lib, n = _lib.lib(), [0, 0]
    fwd, bwd = lib.tzr_cross_fwd, lib.tzr_cross_bwd

    def f(*a):
        n[0] += 1
        return fwd(*a)

    def b(*a):
        n[1] += 1
        return bwd(*a)

    lib.tzr_cross_fwd, lib.tzr_cross_bwd = f, b

    def done():
        lib.tzr_cross_fwd, lib.tzr_cross_bwd = fwd, bwd
        return tuple(n)

    return done


@pytest.mark.parametrize("B,D,L", EDGES)
def test_kernel_edges(dev, B, D, L):
    x, ws, bs, gy = ref.draw(B, D, L, seed=B * 131 + D)
    want = ref.cross_literal(x, ws, bs, gy)
    gaps = ref.literal_gaps(x, ws, bs, gy, want)
    m = _module(dev, D, ws, bs)
    got = _run_module(m, x.to(dev), gy.to(dev))
    ref.check(got, want, gaps, f"({B}, {D}, {L}) on {dev.type}")
    again = _run_module(m, x.to(dev), gy.to(dev))
    assert _bit_equal(got, again), "two runs of the same case differ"


def test_rows_inside_wider_tensors(dev):
    """(300, 48, 3): x and gy are column slices of wider tensors (row stride 52), x one float behind a 16-byte boundary"""
    B, D, L = 300, 48, 3
    x, ws, bs, gy = ref.draw(B, D, L, seed=7)
    want = ref.cross_literal(x, ws, bs, gy)
    gaps = ref.literal_gaps(x, ws, bs, gy, want)
    xw = torch.full((B, 52), float("nan"), device=dev)
    gw = torch.full((B, 52), float("nan"), device=dev)
    xw[:, 1:49], gw[:, 4:52] = x.to(dev), gy.to(dev)
    xv, gv = xw[:, 1:49], gw[:, 4:52]
    assert xv.stride(0) == 52 and xv.data_ptr() % 16 == 4 and gv.stride(0) == 52
    ws_d, bs_d = [w.to(dev) for w in ws], [b.to(dev) for b in bs]
    got = _run_library(dev, xv, ws_d, bs_d, gv)
    ref.check(got, want, gaps, f"strided ({B}, {D}, {L}) on {dev.type}")
    assert _bit_equal(got, _run_library(dev, xv, ws_d, bs_d, gv))
    # the module takes the slice as it lies (no copy) and computes the same bits as on a contiguous copy
    m = _module(dev, D, ws, bs)
    calls = _count_calls()
    a = _run_module(m, xv, gv)
    assert calls() == (1, 1)
    assert _bit_equal(a, got) and _bit_equal(a, _run_module(m, xv.contiguous(), gv.contiguous()))
    # an expanded gradient (every row the same memory) is copied to rows first
    y = m(xv.detach().clone().requires_grad_(True))
    y.sum().backward()
    assert bool(torch.isfinite(m.b[0].grad).all())


@pytest.mark.parametrize("how", ["switch", "wide", "deep"])
def test_literal_loop_outside_the_kernels_limits(dev, monkeypatch, how):
    B, D, L = {"switch": (12, 40, 3), "wide": (3, 1025, 2), "deep": (4, 24, 9)}[how]
    if how == "switch":
        monkeypatch.setattr(interaction, "FUSED_CROSS", False)
    x, ws, bs, gy = ref.draw(B, D, L, seed=11)
    want = ref.cross_literal(x, ws, bs, gy)
    gaps = ref.literal_gaps(x, ws, bs, gy, want)
    m = _module(dev, D, ws, bs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (0, 0)
    ref.check(got, want, gaps, f"literal loop ({how}) on {dev.type}")


def test_empty_batch_and_no_layer_never_reach_the_library(dev):
    calls = _count_calls()
    m = Cross(20, 3).to(dev)
    x = torch.zeros(0, 20, device=dev, requires_grad=True)
    y = m(x)
    y.sum().backward()
    assert y.shape == (0, 20) and x.grad.shape == (0, 20)
    assert all(float(l.weight.grad.abs().sum()) == 0.0 for l in m.w)
    m0 = Cross(20, 0).to(dev)
    assert m0.output_dim() == 20 and list(m0.state_dict()) == []
    x = torch.randn(5, 20, device=dev, requires_grad=True)
    y = m0(x)
    assert torch.equal(y, x)
    y.sum().backward()
    assert torch.equal(x.grad, torch.ones_like(x))
    assert calls() == (0, 0)


def test_parameters_are_the_references():
    m = Cross(13)
    assert m.cross_num == 3 and m.output_dim() == 13
    assert list(m.state_dict()) == ["w.0.weight", "w.1.weight", "w.2.weight", "b.0", "b.1", "b.2"]
    assert all(l.weight.shape == (1, 13) and l.bias is None for l in m.w) and all(b.shape == (13,) for b in m.b)
    bound = (6.0 / 14) ** 0.5
    assert all(float(b.detach().abs().max()) == 0.0 for b in m.b) and all(0 < float(l.weight.detach().abs().max()) <= bound for l in m.w)
