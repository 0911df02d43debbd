"""`CrossV2` (torcheasyrec_amd/interaction.py) on tzr_cross_v2_fwd / tzr_cross_v2_bwd (csrc/cross_v2.hip): against the
reference's own module (tests/golden/reference_cross_v2_vectors.npz) and, at the kernels' edges, against the float64
restatement of the literal loop (tests/cross_v2_ref.py).

Bound, per tensor kind (y, gx, gu, gv, gc; a kind takes the layers together): |ours - fp64| / max(1, |fp64|) <=
max(4 x gap, 2^-20), gap = the distance of the reference's (for the edge cases: torch's literal fp32 form's) result to
float64 on the same inputs -- never anything the code under test computed.  The factor 4 is the one tests/test_cross_net.py
and tests/test_losses.py use.

Measured ours / literal (err / gap, printed per case and kind), minimum - maximum over the three .npz cases, the ten edges and
the strided case; the degenerate (1, 1, 1, 1) edge, whose errors of 3e-9 lie under the floor, left out:
    emulator   y 0.63 - 1.51   gx 0.54 - 1.25   gu 0.12 - 1.29   gv 0.27 - 1.57   gc 0.58 - 1.14
    MI355X     y 0.62 - 1.29   gx 0.52 - 1.24   gu 0.21 - 0.66   gv 0.27 - 1.38   gc 0.42 - 1.14
Two orders were fixed to get there (csrc/cross_v2.hip says where): with `g + dt U_l` as one accumulator chain started at g,
(3, 1024, 64, 8) measured gc 5.4, gx 3.2, gv 2.9; with one chain per lane for dc_l, (8229, 33, 8, 2) measured gc 5.1."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cross_v2_ref as ref
from torcheasyrec_amd import _lib
from torcheasyrec_amd import interaction
from torcheasyrec_amd.interaction import CrossV2

VEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_cross_v2_vectors.npz"))
NPZ_CASES = {"b6_d33_r3_l3": (6, 33, 3, 3), "b21_d429_r32_l2": (21, 429, 32, 2), "b9_d64_r16_l1": (9, 64, 16, 1)}
ROWS, MAXGRID = 16, 512  # CV_ROWS, CV_MAXGRID of csrc/cross_v2.hip: a launch holds at most 512 blocks of 16 rows at a time
CONCURRENT = ROWS * MAXGRID
CLASSES = (256, 512, 1024)  # the D classes of the row kernels' templates
EDGES = [(1, 1, 1, 1), (5, 33, 3, 2), (17, 65, 17, 3), (33, 429, 32, 3), (3, 1024, 64, 8), (4, 256, 8, 2), (4, 257, 8, 2), (4, 512, 5, 1),
         (4, 513, 5, 1), (CONCURRENT + 37, 33, 8, 2)]


def _module(dev, D, us, vs, cs):
    m = CrossV2(D, len(us), us[0].shape[0] if us else 4)
    with torch.no_grad():
        for i, (u, v, c) in enumerate(zip(us, vs, cs)):
            m.u_kernels[i].weight.copy_(u)
            m.v_kernels[i].weight.copy_(v)
            m.v_kernels[i].bias.copy_(c)
    return m.to(dev)


def _run_module(m, x, gy):
    for p in m.parameters():
        p.grad = None
    x = x.detach().clone().requires_grad_(True)
    y = m(x)
    y.backward(gy)
    return {"y": [y.detach()], "gx": [x.grad], "gu": [l.weight.grad for l in m.u_kernels], "gv": [l.weight.grad for l in m.v_kernels],
            "gc": [l.bias.grad for l in m.v_kernels]}


def _run_library(dev, x, us, vs, cs, gy, save=True):
    """the two entry points on the tensors as they lie (x and gy may be column slices of wider tensors)"""
    lib, L, (B, D), R = _lib.lib(), len(us), x.shape, us[0].shape[0]
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    y, xs, t, dx, du, dv, dc = new(B, D), new(max(L - 1, 1), B, D), new(L, B, R), new(B, D), new(L, R, D), new(L, D, R), new(L, D)
    pu, pv, pc = ((C.c_void_p * L)(*[_lib.ptr(p) for p in ps]) for ps in (us, vs, cs))
    st = _lib.stream_ptr(dev)
    assert lib.tzr_cross_v2_fwd(_lib.ptr(x), x.stride(0), pu, pv, pc, L, B, D, R, _lib.ptr(y), D, _lib.ptr(xs) if save else None,
                                _lib.ptr(t) if save else None, st) == 0
    if not save:
        return {"y": [y]}
    wsp = _lib.workspace(lib.tzr_cross_v2_bwd_workspace(B, D, R, L), dev)
    assert lib.tzr_cross_v2_bwd(_lib.ptr(gy), gy.stride(0), _lib.ptr(x), x.stride(0), _lib.ptr(xs), _lib.ptr(t), pu, pv, pc, L, B, D, R,
                                _lib.ptr(dx), D, _lib.ptr(du), _lib.ptr(dv), _lib.ptr(dc), _lib.ptr(wsp), wsp.numel(), st) == 0
    return {"y": [y], "gx": [dx], "gu": list(du), "gv": list(dv), "gc": list(dc)}


def _bit_equal(a, b):
    return all(torch.equal(p.reshape(-1), q.reshape(-1)) for k in ref.KINDS for p, q in zip(a[k], b[k]))


def _count_calls():
    """(forward, backward) calls of the library since this call; restored by the `dev` fixture's next use_library"""
    lib, n = _lib.lib(), [0, 0]
    fwd, bwd = lib.tzr_cross_v2_fwd, lib.tzr_cross_v2_bwd

    def f(*a):
        n[0] += 1
        return fwd(*a)

    def b(*a):
        n[1] += 1
        return bwd(*a)

    lib.tzr_cross_v2_fwd, lib.tzr_cross_v2_bwd = f, b

    def done():
        lib.tzr_cross_v2_fwd, lib.tzr_cross_v2_bwd = fwd, bwd
        return tuple(n)

    return done


@pytest.mark.parametrize("tag", list(NPZ_CASES))
def test_module_matches_the_reference_module(dev, monkeypatch, tag):
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", True)
    B, D, R, L = NPZ_CASES[tag]
    x, gy = torch.from_numpy(VEC[f"{tag}/x"]), torch.from_numpy(VEC[f"{tag}/gy"])
    us, vs, cs = ([torch.from_numpy(VEC[f"{tag}/{n}{i}"]) for i in range(L)] for n in "uvc")
    assert x.shape == (B, D) and us[0].shape == (R, D) and vs[0].shape == (D, R) and all(float(c.abs().max()) > 0 for c in cs)
    want = ref.literal(x, us, vs, cs, gy)
    gaps = {k: float(VEC[f"ref_gap/{tag}/{k}"]) for k in ref.KINDS}
    # the stored results are the reference's: the restatement reproduces them to the stored gap
    stored = {"y": [torch.from_numpy(VEC[f"{tag}/y"])], "gx": [torch.from_numpy(VEC[f"{tag}/gx"])]}
    for n in ("gu", "gv", "gc"):
        stored[n] = [torch.from_numpy(VEC[f"{tag}/{n}{i}"]) for i in range(L)]
    for k in ref.KINDS:
        assert abs(ref.rel_err(stored[k], want[k]) - gaps[k]) <= 1e-12, k
    m = _module(dev, D, us, vs, cs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (1, 1)  # exactly one forward and one backward library call per step
    ref.check(got, want, gaps, f"{tag} on {dev.type}")
    assert got["gu"][0].shape == (R, D) and got["gv"][0].shape == (D, R) and got["gc"][0].shape == (D,)


@pytest.mark.parametrize("B,D,R,L", EDGES)
def test_kernel_edges(dev, monkeypatch, B, D, R, L):
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", True)
    x, us, vs, cs, gy = ref.draw(B, D, R, L, seed=B * 131 + D)
    want = ref.literal(x, us, vs, cs, gy)
    gaps = ref.literal_gaps(x, us, vs, cs, gy, want)
    m = _module(dev, D, us, vs, cs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (1, 1)
    ref.check(got, want, gaps, f"({B}, {D}, {R}, {L}) on {dev.type}")
    again = _run_module(m, x.to(dev), gy.to(dev))
    assert _bit_equal(got, again), "two runs of the same case differ"


def test_the_edges_take_every_tail_class_border_and_an_uneven_wrap():
    assert (1, 1, 1, 1) in EDGES and (5, 33, 3, 2) in EDGES and (33, 429, 32, 3) in EDGES and (3, 1024, 64, 8) in EDGES
    B, D, R, L = EDGES[2]  # one row over a 16-row block, one column over a tile, r one over a tile
    assert (B % ROWS, D % 16, R % 16) == (1, 1, 1) and B > ROWS and L == 3
    for border in CLASSES[:-1]:  # one shape on each side of every border between two D classes
        assert any(s[1] == border for s in EDGES) and any(s[1] == border + 1 for s in EDGES)
    assert max(s[1] for s in EDGES) == CLASSES[-1] == interaction.CROSS_V2_MAX_DIM
    assert max(s[2] for s in EDGES) == interaction.CROSS_V2_MAX_RANK and max(s[3] for s in EDGES) == interaction.CROSS_V2_MAX_LAYERS
    B = EDGES[-1][0]  # the grid-stride loop wraps, and unevenly: some workgroups take a second block, one of them a partial one
    assert B == CONCURRENT + 37 and 0 < -(-B // ROWS) - MAXGRID < MAXGRID and B % ROWS != 0


def test_rows_inside_wider_tensors(dev, monkeypatch):
    """(37, 45, 6, 3): x, gy and the outputs of the library are column slices of wider NaN-filled tensors with an odd row
    stride (53), x one float behind a 16-byte boundary"""
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", True)
    B, D, R, L = 37, 45, 6, 3
    x, us, vs, cs, gy = ref.draw(B, D, R, L, seed=7)
    want = ref.literal(x, us, vs, cs, gy)
    gaps = ref.literal_gaps(x, us, vs, cs, gy, want)
    nan = float("nan")
    xw, gw = torch.full((B, 53), nan, device=dev), torch.full((B, 53), nan, device=dev)
    xw[:, 1:46], gw[:, 4:49] = x.to(dev), gy.to(dev)
    xv, gv = xw[:, 1:46], gw[:, 4:49]
    assert xv.stride(0) == 53 and xv.data_ptr() % 16 == 4 and gv.stride(0) == 53
    us_d, vs_d, cs_d = ([p.to(dev) for p in ps] for ps in (us, vs, cs))
    got = _run_library(dev, xv, us_d, vs_d, cs_d, gv)
    ref.check(got, want, gaps, f"strided ({B}, {D}, {R}, {L}) on {dev.type}")
    assert _bit_equal(got, _run_library(dev, xv, us_d, vs_d, cs_d, gv))
    # strided outputs: nothing outside the slices is written
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    yw, dxw = torch.full((B, 53), nan, device=dev), torch.full((B, 53), nan, device=dev)
    xs, t = torch.empty(L - 1, B, D, device=dev), torch.empty(L, B, R, device=dev)
    du, dv, dc = torch.empty(L, R, D, device=dev), torch.empty(L, D, R, device=dev), torch.empty(L, D, device=dev)
    pu, pv, pc = ((C.c_void_p * L)(*[_lib.ptr(p) for p in ps]) for ps in (us_d, vs_d, cs_d))
    assert lib.tzr_cross_v2_fwd(_lib.ptr(xv), 53, pu, pv, pc, L, B, D, R, _lib.ptr(yw[:, 3:48]), 53, _lib.ptr(xs), _lib.ptr(t), st) == 0
    wsp = _lib.workspace(lib.tzr_cross_v2_bwd_workspace(B, D, R, L), dev)
    assert lib.tzr_cross_v2_bwd(_lib.ptr(gv), 53, _lib.ptr(xv), 53, _lib.ptr(xs), _lib.ptr(t), pu, pv, pc, L, B, D, R, _lib.ptr(dxw[:, 5:50]), 53,
                                _lib.ptr(du), _lib.ptr(dv), _lib.ptr(dc), _lib.ptr(wsp), wsp.numel(), st) == 0
    assert torch.equal(yw[:, 3:48], got["y"][0]) and torch.equal(dxw[:, 5:50], got["gx"][0])
    assert bool(torch.isnan(yw[:, :3]).all()) and bool(torch.isnan(yw[:, 48:]).all())
    assert bool(torch.isnan(dxw[:, :5]).all()) and bool(torch.isnan(dxw[:, 50:]).all())
    assert bool(torch.isnan(xw[:, :1]).all()) and bool(torch.isnan(xw[:, 46:]).all()) and torch.equal(xw[:, 1:46], x.to(dev))
    # the module takes the slice as it lies (no copy) and computes the same bits as on a contiguous copy
    m = _module(dev, D, us, vs, cs)
    calls = _count_calls()
    a = _run_module(m, xv, gv)
    assert calls() == (1, 1)
    assert _bit_equal(a, got) and _bit_equal(a, _run_module(m, xv.contiguous(), gv.contiguous()))
    # an expanded gradient (every row the same memory) is copied to rows first
    m.zero_grad(set_to_none=True)
    y = m(xv.detach().clone().requires_grad_(True))
    y.sum().backward()
    assert bool(torch.isfinite(m.v_kernels[0].bias.grad).all())
    want_gc = ref.literal(x, us, vs, cs, torch.ones(B, D))
    assert ref.rel_err([l.bias.grad for l in m.v_kernels], want_gc["gc"]) <= 1e-4


def test_the_module_passes_the_slice_without_a_copy(dev, monkeypatch):
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", True)
    B, D, R, L = 5, 20, 4, 2
    x, us, vs, cs, gy = ref.draw(B, D, R, L, seed=3)
    xw = torch.full((B, 27), float("nan"), device=dev)
    xw[:, 2:22] = x.to(dev)
    xv = xw[:, 2:22].detach().requires_grad_(True)
    m = _module(dev, D, us, vs, cs)
    lib, seen = _lib.lib(), []
    fwd = lib.tzr_cross_v2_fwd
    lib.tzr_cross_v2_fwd = lambda *a: (seen.append((a[0], a[1])), fwd(*a))[1]
    try:
        m(xv)
    finally:
        lib.tzr_cross_v2_fwd = fwd
    assert seen == [(xv.data_ptr(), 27)]


@pytest.mark.parametrize("how", ["switch", "wide", "rank", "deep"])
def test_literal_loop_outside_the_kernels_limits(dev, monkeypatch, how):
    B, D, R, L = {"switch": (12, 40, 8, 3), "wide": (3, 1025, 4, 2), "rank": (4, 24, 65, 2), "deep": (4, 24, 4, 9)}[how]
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", how != "switch")
    x, us, vs, cs, gy = ref.draw(B, D, R, L, seed=11)
    want = ref.literal(x, us, vs, cs, gy)
    gaps = ref.literal_gaps(x, us, vs, cs, gy, want)
    m = _module(dev, D, us, vs, cs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (0, 0)
    ref.check(got, want, gaps, f"literal loop ({how}) on {dev.type}")


def test_empty_batch_and_no_layer_never_reach_the_library(dev, monkeypatch):
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", True)
    calls = _count_calls()
    m = CrossV2(20, 3, 4).to(dev)
    x = torch.zeros(0, 20, device=dev, requires_grad=True)
    y = m(x)
    y.sum().backward()
    assert y.shape == (0, 20) and x.grad.shape == (0, 20)
    assert all(float(l.weight.grad.abs().sum()) == 0.0 for l in m.u_kernels)
    m0 = CrossV2(20, 0, 4).to(dev)
    assert m0.output_dim() == 20 and list(m0.state_dict()) == []
    x = torch.randn(5, 20, device=dev, requires_grad=True)
    y = m0(x)
    assert torch.equal(y, x)
    y.sum().backward()
    assert torch.equal(x.grad, torch.ones_like(x))
    assert calls() == (0, 0)


def test_parameters_are_the_references():
    m = CrossV2(13)
    assert m.cross_num == 3 and m.output_dim() == 13
    assert list(m.state_dict()) == ["u_kernels.0.weight", "u_kernels.1.weight", "u_kernels.2.weight", "v_kernels.0.weight", "v_kernels.0.bias",
                                    "v_kernels.1.weight", "v_kernels.1.bias", "v_kernels.2.weight", "v_kernels.2.bias"]
    assert all(l.weight.shape == (32, 13) and l.bias is None for l in m.u_kernels)
    assert all(l.weight.shape == (13, 32) and l.bias.shape == (13,) for l in m.v_kernels)
    # nn.Linear's default: kaiming_uniform(a = sqrt 5) = U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for the weight and the bias
    bu, bv = 13 ** -0.5, 32 ** -0.5
    assert all(0 < float(l.weight.detach().abs().max()) <= bu for l in m.u_kernels)
    assert all(0 < float(l.weight.detach().abs().max()) <= bv and 0 < float(l.bias.detach().abs().max()) <= bv for l in m.v_kernels)
    m = CrossV2(7, cross_num=2, low_rank=5)
    assert m.u_kernels[1].weight.shape == (5, 7) and m.v_kernels[1].weight.shape == (7, 5) and len(m.u_kernels) == 2


@pytest.mark.parametrize("B,D,R,L", [(19, 70, 9, 3), (5, 300, 32, 1)])
def test_inference_forward_has_the_training_forwards_bits(dev, monkeypatch, B, D, R, L):
    monkeypatch.setattr(interaction, "FUSED_CROSS_V2", True)
    x, us, vs, cs, gy = ref.draw(B, D, R, L, seed=5)
    xd, gd = x.to(dev), gy.to(dev)
    us_d, vs_d, cs_d = ([p.to(dev) for p in ps] for ps in (us, vs, cs))
    train = _run_library(dev, xd, us_d, vs_d, cs_d, gd)["y"][0]
    assert torch.equal(_run_library(dev, xd, us_d, vs_d, cs_d, gd, save=False)["y"][0], train)
    # the module under no_grad passes null save pointers
    m = _module(dev, D, us, vs, cs)
    lib, seen = _lib.lib(), []
    fwd = lib.tzr_cross_v2_fwd
    lib.tzr_cross_v2_fwd = lambda *a: (seen.append((a[11], a[12])), fwd(*a))[1]
    try:
        with torch.no_grad():
            y = m(xd)
    finally:
        lib.tzr_cross_v2_fwd = fwd
    assert seen == [(None, None)] and torch.equal(y, train)
