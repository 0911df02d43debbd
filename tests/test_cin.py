"""`CIN` (torcheasyrec_amd/interaction.py) on tzr_cin_fwd / tzr_cin_bwd (csrc/cin.hip): against the reference's own module
(tests/golden/reference_cin_vectors.npz) and, at the kernels' edges, against the float64 restatement of the literal loop
(tests/cin_ref.py).

Bound, per tensor kind (y, gx, gw, gb): |ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the LARGER of two fp32
evaluations' distances to float64 on the same inputs -- the literal form (for the npz cases: the reference's stored one) and
the factored form of tests/cin_ref.py -- never anything the code under test computed.  The factor 4 and the floor are the
ones tests/cross_ref.py and tests/test_losses.py use."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cin_ref as ref
from torcheasyrec_amd import _lib
from torcheasyrec_amd import interaction
from torcheasyrec_amd.interaction import CIN

VEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_cin_vectors.npz"))
NPZ_CASES = {"b5_f3_d16": (5, 3, 16, [8, 4, 2]), "b37_f26_d16": (37, 26, 16, [32, 24]), "b9_f39_d8": (9, 39, 8, [20, 17, 1])}
# A launch of the forward holds at most CIN_MAXGRID = 1024 workgroups x (32 // D) samples at a time, one of the input-gradient
# kernel 1024 workgroups x 32 columns (csrc/cin.hip): at D = 8 that is 4096 samples either way.
MAXGRID, COLUMNS, LOOP_D = 1024, 32, 8
CONCURRENT = MAXGRID * (COLUMNS // LOOP_D)
EDGES = [(1, 1, 1, [1]), (70, 7, 5, [17, 1]), (33, 2, 64, [16]), (3, 64, 4, [256]), (6, 5, 16, [16, 16, 16, 16]),
         (CONCURRENT + 1, 3, LOOP_D, [4])]


def _module(dev, F, layers, ws, bs):
    m = CIN(F, layers)
    with torch.no_grad():
        for l, w, b in zip(m.cin_layers, ws, bs):
            l.weight.copy_(w)
            l.bias.copy_(b)
    return m.to(dev)


def _run_module(m, x, gy):
    for p in m.parameters():
        p.grad = None
    x = x.detach().requires_grad_(True) if x.is_contiguous() else x.detach().clone().requires_grad_(True)
    y = m(x)
    y.backward(gy)
    return {"y": [y.detach()], "gx": [x.grad], "gw": [l.weight.grad for l in m.cin_layers], "gb": [l.bias.grad for l in m.cin_layers]}


def _run_library(dev, x2, F, D, layers, ws, bs, gy, gx):
    """the entry points on the tensors as they lie: x2 [B, F D], gy and gx may be column slices of wider tensors"""
    lib, L, B = _lib.lib(), len(layers), x2.shape[0]
    hs = [F] + layers[:-1]
    y = torch.empty(B, sum(layers), dtype=torch.float32, device=dev)
    xs = [torch.empty(B, o, D, dtype=torch.float32, device=dev) for o in layers[:-1]]
    dwc = torch.empty(sum(o * h * F + o for o, h in zip(layers, hs)), dtype=torch.float32, device=dev)
    arr = lambda ts: (C.c_void_p * max(1, len(ts)))(*[_lib.ptr(t) for t in ts])  # noqa: E731
    sizes, st = (C.c_int * L)(*layers), _lib.stream_ptr(dev)
    assert lib.tzr_cin_fwd(_lib.ptr(x2), x2.stride(0), arr(ws), arr(bs), sizes, L, B, F, D, arr(xs), _lib.ptr(y), y.shape[1], st) == 0
    wsp = _lib.workspace(lib.tzr_cin_bwd_workspace(B, F, D, sizes, L), dev)
    assert lib.tzr_cin_bwd(_lib.ptr(gy), gy.stride(0), _lib.ptr(x2), x2.stride(0), arr(ws), sizes, L, B, F, D, arr(xs), _lib.ptr(gx),
                           gx.stride(0), _lib.ptr(dwc), _lib.ptr(wsp), wsp.numel(), st) == 0
    gws, gbs, off = [], [], 0
    for o, h in zip(layers, hs):
        gws.append(dwc[off:off + o * h * F].clone())
        gbs.append(dwc[off + o * h * F:off + o * h * F + o].clone())
        off += o * h * F + o
    return {"y": [y], "gx": [gx.clone()], "gw": gws, "gb": gbs}


def _bit_equal(a, b):
    return all(torch.equal(p.reshape(-1), q.reshape(-1)) for k in ref.KINDS for p, q in zip(a[k], b[k]))


def _count_calls():
    """(forward, backward) calls of the library since this call; restored by the `dev` fixture's next use_library"""
    lib, n = _lib.lib(), [0, 0]
    fwd, bwd = lib.tzr_cin_fwd, lib.tzr_cin_bwd

    def f(*a):
        n[0] += 1
        return fwd(*a)

    def b(*a):
        n[1] += 1
        return bwd(*a)

    lib.tzr_cin_fwd, lib.tzr_cin_bwd = f, b

    def done():
        lib.tzr_cin_fwd, lib.tzr_cin_bwd = fwd, bwd
        return tuple(n)

    return done


@pytest.mark.parametrize("tag", list(NPZ_CASES))
def test_module_matches_the_reference_module(dev, tag):
    B, F, D, layers = NPZ_CASES[tag]
    L = len(layers)
    x, gy = torch.from_numpy(VEC[f"{tag}/x"]), torch.from_numpy(VEC[f"{tag}/gy"])
    ws = [torch.from_numpy(VEC[f"{tag}/w{i}"]) for i in range(L)]
    bs = [torch.from_numpy(VEC[f"{tag}/b{i}"]) for i in range(L)]
    assert x.shape == (B, F, D) and all(float(b.abs().max()) > 0 for b in bs)
    want = ref.cin_literal(x, ws, bs, gy)
    stored_gaps = {k: float(VEC[f"ref_gap/{tag}/{k}"]) for k in ref.KINDS}
    # the stored results are the reference's: the restatement reproduces them to the stored gap
    stored = {"y": [torch.from_numpy(VEC[f"{tag}/y"])], "gx": [torch.from_numpy(VEC[f"{tag}/gx"])],
              "gw": [torch.from_numpy(VEC[f"{tag}/gw{i}"]) for i in range(L)], "gb": [torch.from_numpy(VEC[f"{tag}/gb{i}"]) for i in range(L)]}
    for k in ref.KINDS:
        assert abs(ref.rel_err(stored[k], want[k]) - stored_gaps[k]) <= 1e-12, k
    gaps = ref.form_gaps(x, ws, bs, gy, want, stored=stored_gaps)
    m = _module(dev, F, layers, ws, bs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (1, 1)
    ref.check(got, want, gaps, f"{tag} on {dev.type}")
    assert got["gw"][0].shape == (layers[0], F * F, 1) and got["gb"][0].shape == (layers[0],)


@pytest.mark.parametrize("B,F,D,layers", EDGES)
def test_kernel_edges(dev, B, F, D, layers):
    x, ws, bs, gy = ref.draw(B, F, D, layers, seed=B * 131 + F * 7 + D)
    want = ref.cin_literal(x, ws, bs, gy)
    gaps = ref.form_gaps(x, ws, bs, gy, want)
    m = _module(dev, F, layers, ws, bs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (1, 1)
    ref.check(got, want, gaps, f"({B}, {F}, {D}, {layers}) on {dev.type}")
    again = _run_module(m, x.to(dev), gy.to(dev))
    assert _bit_equal(got, again), "two runs of the same case differ"


def test_input_inside_a_wider_tensor(dev):
    """(21, 5, 12, [9, 6]): x and gx are column slices of wider tensors (row stride F D + 4), one float behind a 16-byte
    boundary, NaN outside the slice"""
    B, F, D, layers = 21, 5, 12, [9, 6]
    x, ws, bs, gy = ref.draw(B, F, D, layers, seed=7)
    want = ref.cin_literal(x, ws, bs, gy)
    gaps = ref.form_gaps(x, ws, bs, gy, want)
    W = F * D + 4
    xw = torch.full((B, W), float("nan"), device=dev)
    gxw = torch.full((B, W), float("nan"), device=dev)
    xw[:, 1:1 + F * D] = x.reshape(B, F * D).to(dev)
    xv, gxv = xw[:, 1:1 + F * D], gxw[:, 1:1 + F * D]
    assert xv.stride(0) == W and xv.data_ptr() % 16 == 4 and gxv.data_ptr() % 16 == 4
    ws_d, bs_d, gy_d = [w.to(dev) for w in ws], [b.to(dev) for b in bs], gy.to(dev)
    got = _run_library(dev, xv, F, D, layers, ws_d, bs_d, gy_d, gxv)
    ref.check(got, want, gaps, f"strided ({B}, {F}, {D}, {layers}) on {dev.type}")
    outside = torch.cat([gxw[:, :1], gxw[:, 1 + F * D:]], dim=1)
    assert bool(torch.isnan(outside).all()), "a store outside the slice"
    flat = _run_library(dev, xv.contiguous(), F, D, layers, ws_d, bs_d, gy_d, torch.empty(B, F * D, device=dev))
    assert _bit_equal(got, flat), "a slice and its contiguous copy differ"
    # the module takes the [B, F, D] view of the slice as it lies (one call each way) and computes the same bits
    m = _module(dev, F, layers, ws, bs)
    calls = _count_calls()
    a = _run_module(m, xv.view(B, F, D), gy_d)
    assert calls() == (1, 1)
    assert _bit_equal(a, got)
    # an expanded gradient (every row the same memory) is copied to rows first
    y = m(xv.view(B, F, D).detach().clone().requires_grad_(True))
    y.sum().backward()
    assert bool(torch.isfinite(m.cin_layers[0].bias.grad).all())


@pytest.mark.parametrize("how", ["switch", "dim", "features", "layer_size", "layers"])
def test_literal_loop_outside_the_kernels_limits(dev, monkeypatch, how):
    B, F, D, layers = {"switch": (12, 4, 8, [6, 3]), "dim": (3, 2, 65, [4]), "features": (2, 65, 2, [3]), "layer_size": (2, 3, 4, [257, 2]),
                       "layers": (3, 3, 4, [4, 3, 2, 3, 2])}[how]
    if how == "switch":
        monkeypatch.setattr(interaction, "FUSED_CIN", False)
    x, ws, bs, gy = ref.draw(B, F, D, layers, seed=11)
    want = ref.cin_literal(x, ws, bs, gy)
    gaps = ref.form_gaps(x, ws, bs, gy, want)
    m = _module(dev, F, layers, ws, bs)
    calls = _count_calls()
    got = _run_module(m, x.to(dev), gy.to(dev))
    assert calls() == (0, 0)
    ref.check(got, want, gaps, f"literal loop ({how}) on {dev.type}")


def test_empty_batch_never_reaches_the_library(dev):
    calls = _count_calls()
    m = CIN(4, [5, 3]).to(dev)
    x = torch.zeros(0, 4, 8, device=dev, requires_grad=True)
    y = m(x)
    y.sum().backward()
    assert y.shape == (0, 8) and x.grad.shape == (0, 4, 8)
    assert all(float(l.weight.grad.abs().sum()) == 0.0 and float(l.bias.grad.abs().sum()) == 0.0 for l in m.cin_layers)
    assert calls() == (0, 0)


def test_a_second_backward_is_refused(dev):
    """the backward consumes the saved activations: running it again on the same graph is an error, never a wrong result"""
    m = CIN(3, [4, 2]).to(dev)
    y = m(torch.randn(5, 3, 8, device=dev, requires_grad=True))
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="forward again"):
        y.sum().backward()


def test_parameters_are_the_references():
    m = CIN(5, [7, 3])
    assert m.output_dim() == 10 and m.feature_num == 5 and m.cin_layer_size == [7, 3]
    assert list(m.state_dict()) == ["cin_layers.0.weight", "cin_layers.0.bias", "cin_layers.1.weight", "cin_layers.1.bias"]
    assert [tuple(p.shape) for p in m.state_dict().values()] == [(7, 25, 1), (7,), (3, 35, 1), (3,)]
    for l, fan_in in zip(m.cin_layers, (25, 35)):  # Conv1d's default: both within 1 / sqrt(fan_in)
        bound = 1.0 / fan_in ** 0.5
        assert 0 < float(l.weight.detach().abs().max()) <= bound and 0 < float(l.bias.detach().abs().max()) <= bound
