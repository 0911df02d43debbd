"""`WuKongLayer` (torcheasyrec_amd/wukong.py) on the entry points of csrc/wukong.hip against the reference's own module
(tests/golden/reference_wukong_vectors.npz, LayerNorm weights and biases random) and the float64 restatement of the literal
layer (tests/wukong_ref.py).

Bound, per tensor kind: |ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the distance of the reference's stored
result to float64 on the same inputs -- never anything the code under test computed.  Kinds: y, gx and one per parameter
(`g:lcb.weight` and `g:residual_projection.weight` are kinds of their own, though one product yields both).  The stored cases
hold no ReLU pre-activation within 2^-16 of zero (the generator asserts it; checked again here), so no row is left out."""
import os
import re

import numpy as np
import pytest
import torch

import wukong_ref as ref
from torcheasyrec_amd import _lib
from torcheasyrec_amd import wukong
from torcheasyrec_amd.wukong import WuKongLayer

VEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_wukong_vectors.npz"))
# (B, F, D, Fl, Ff, k, mlp)
CASES = {"b6_f3_d8_l3_f4_k2": (6, 3, 8, 3, 4, 2, [4]), "b6_f7_d8_l3_f4_k3": (6, 7, 8, 3, 4, 3, [4]),
         "b9_f27_d128_l16_f16_k24": (9, 27, 128, 16, 16, 24, [16])}
ENTRY_POINTS = ("tzr_wukong_fm_fwd", "tzr_wukong_mix_fwd", "tzr_wukong_fm_bwd", "tzr_wukong_mix_bwd")


def _count_calls():
    """(forward, backward) calls of the four entry points since this call; restored by the `dev` fixture's next use_library"""
    lib, n = _lib.lib(), [0, 0]
    orig = {nm: getattr(lib, nm) for nm in ENTRY_POINTS}

    def counted(nm, slot):
        def f(*a):
            n[slot] += 1
            return orig[nm](*a)
        return f

    for i, nm in enumerate(ENTRY_POINTS):
        setattr(lib, nm, counted(nm, i // 2))

    def done():
        for nm in ENTRY_POINTS:
            setattr(lib, nm, orig[nm])
        return tuple(n)

    return done


def _mine(key):
    """the reference's state-dict key in this package: its MLP's Linear of layer i is `mlp.<i>.perceptron.0`, `MLP`'s is `mlp.<2i>`
    (so for every model built here); everything else is key for key the reference's"""
    return re.sub(r"\.mlp\.mlp\.(\d+)\.perceptron\.0\.", lambda m: f".mlp.mlp.{2 * int(m.group(1))}.", key)


def _load(tag):
    keys = [str(k) for k in VEC[f"keys/{tag}"]]
    sd = {k: torch.from_numpy(VEC[f"{tag}/p:{k}"]) for k in keys}
    x, gy = torch.from_numpy(VEC[f"{tag}/x"]), torch.from_numpy(VEC[f"{tag}/gy"])
    names = ["y", "gx"] + [f"g:{k}" for k in keys]
    want = ref.layer_literal(x, sd, gy)
    assert not want.pop("kink")
    gaps = {n: float(VEC[f"ref_gap/{tag}/{n}"]) for n in names}
    for n in names:  # the stored results are the reference's: the restatement reproduces them to the stored gap
        assert abs(ref.rel_err([torch.from_numpy(VEC[f"{tag}/{n}"])], want[n]) - gaps[n]) <= 1e-12, n
    return x, gy, sd, keys, names, want, gaps


def _module(dev, tag, sd):
    B, Fn, D, Fl, Ff, k, mlp = CASES[tag]
    m = WuKongLayer(D, Fn, Fl, Ff, k, {"hidden_units": mlp})
    m.load_state_dict({_mine(key): v for key, v in sd.items()}, strict=True)
    return m.to(dev)


def _run(m, x, gy, keys=None):
    """-> name -> [tensor], the gradients under the reference's keys when `keys` lists them"""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    y = m(x)
    y.backward(gy)
    out = {"y": [y.detach()], "gx": [x.grad]}
    params = dict(m.named_parameters())
    for key in (keys if keys is not None else list(params)):
        out[f"g:{key}"] = [params[_mine(key)].grad]
    return out


@pytest.mark.parametrize("tag", list(CASES))
def test_layer_matches_the_reference_module(dev, tag):
    B, Fn, D, Fl, Ff, k, mlp = CASES[tag]
    x, gy, sd, keys, names, want, gaps = _load(tag)
    projection = Fn != Fl + Ff
    assert ("residual_projection.weight" in keys) == projection and len(names) == 2 + 10 + projection and "g:lcb.weight" in names
    m = _module(dev, tag, sd)
    assert list(m.state_dict()) == [_mine(key) for key in keys]
    assert [key for key in keys if ".mlp.mlp." not in key] == [key for key in m.state_dict() if ".mlp.mlp." not in key]
    assert m.output_feature_num() == Fl + Ff
    assert all(float((sd[key] - (1.0 if key.endswith("weight") else 0.0)).abs().max()) > 0 for key in keys if "norm" in key)
    calls = _count_calls()
    got = _run(m, x.to(dev), gy.to(dev), keys)
    assert calls() == (2, 2)
    assert got["y"][0].shape == (B, Fl + Ff, D)
    ref.check(got, want, gaps, f"{tag} on {dev.type}", names)
    again = _run(m, x.to(dev), gy.to(dev), keys)
    assert all(torch.equal(a, b) for n in names for a, b in zip(got[n], again[n])), "two runs of the same case differ"


@pytest.mark.parametrize("tag", list(CASES))
def test_switch_off_runs_the_literal_forward(dev, monkeypatch, tag):
    """no entry point is called, and the result is torch's literal one bit for bit: the reference's forward, written out here"""
    monkeypatch.setattr(wukong, "FUSED_WUKONG", False)
    x, gy, sd, keys, names, want, gaps = _load(tag)
    m = _module(dev, tag, sd)
    calls = _count_calls()
    got = _run(m, x.to(dev), gy.to(dev), keys)
    assert calls() == (0, 0)

    def literal(inputs):
        f = m.fmb
        o = torch.matmul(inputs, torch.matmul(inputs.permute(0, 2, 1), f.weight))
        o = f.feature_out_liner(f.mlp(f.norm(o.view(-1, f.feature_num_in * f.compressed_feature_num)))).view(-1, f.feature_num_out, f.input_dim)
        lcb = (inputs.permute(0, 2, 1) @ m.lcb.weight).permute(0, 2, 1)
        return m.norm(torch.concat((o, lcb), dim=1) + m.residual_projection(inputs))

    m.zero_grad(set_to_none=True)
    xl = x.to(dev).clone().requires_grad_(True)
    y = literal(xl)
    y.backward(gy.to(dev))
    params = dict(m.named_parameters())
    assert torch.equal(y.detach(), got["y"][0]) and torch.equal(xl.grad, got["gx"][0])
    assert all(torch.equal(params[_mine(key)].grad, got[f"g:{key}"][0]) for key in keys)
    if dev.type == "cpu":  # (the stored results are the reference's on the CPU)
        ref.check(got, want, gaps, f"literal {tag}", names)


@pytest.mark.parametrize("how", ["double", "wide", "many", "compressed"])
def test_literal_forward_outside_the_kernels_limits(dev, how):
    Fn, D, Fl, Ff, k, dtype = {"double": (5, 8, 3, 4, 2, torch.float64), "wide": (5, 129, 3, 4, 2, torch.float32),
                               "many": (65, 8, 3, 4, 2, torch.float32), "compressed": (5, 8, 3, 4, 65, torch.float32)}[how]
    torch.manual_seed(5)
    m = WuKongLayer(D, Fn, Fl, Ff, k, {"hidden_units": [6]}).to(dev).to(dtype)
    calls = _count_calls()
    x = torch.randn(4, Fn, D, dtype=dtype, device=dev, requires_grad=True)
    y = m(x)
    y.sum().backward()
    assert calls() == (0, 0) and y.shape == (4, Fl + Ff, D) and y.dtype == dtype and bool(torch.isfinite(x.grad).all())


def test_two_layers(dev, monkeypatch):
    """a projection layer into an identity layer (autograd adds the two input gradients of each); gap = the literal fp32 form's
    distance to a float64 run of the literal form, both on the CPU"""
    def twin(dtype):
        t = torch.nn.Sequential(WuKongLayer(20, 5, 3, 4, 3, {"hidden_units": [12]}), WuKongLayer(20, 7, 4, 3, 3, {"hidden_units": [12]})).to(dtype)
        t.load_state_dict({key: v.detach().cpu().to(dtype) for key, v in m.state_dict().items()})
        return t

    torch.manual_seed(11)
    m = torch.nn.Sequential(WuKongLayer(20, 5, 3, 4, 3, {"hidden_units": [12]}), WuKongLayer(20, 7, 4, 3, 3, {"hidden_units": [12]}))
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.3 * torch.randn(mod.weight.shape))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape))
    m = m.to(dev)
    x, gy = torch.randn(9, 5, 20), torch.randn(9, 7, 20)
    calls = _count_calls()
    got = _run(m, x.to(dev), gy.to(dev))
    assert calls() == (4, 4)
    monkeypatch.setattr(wukong, "FUSED_WUKONG", False)
    want = _run(twin(torch.float64), x.double(), gy.double())
    lit = _run(twin(torch.float32), x, gy)
    kinds = list(got)
    ref.check(got, want, {n: ref.rel_err(lit[n], want[n]) for n in kinds}, f"two layers on {dev.type}", kinds)
