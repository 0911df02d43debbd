"""personalized_net.EPNet / PPNet against vectors recorded from the reference's own modules
(tests/golden/make_reference_pepnet_vectors.py running tzrec/modules/personalized_net.py): loaded with the reference's parameters
under the reference's state-dict keys they reproduce the reference's outputs, input gradients and parameter gradients, with the
gate-and-scale step fused (gate_ops.gate_scale: one tzr_gate_scale_fwd per PPNet level, one per EPNet) and in the literal form.
Bound per kind: 4 x the reference's own fp32-vs-float64 distance stored with the vectors, floor 2^-20 (tests/test_ple_module.py's)."""
import os

import numpy as np
import pytest
import torch

from cross_v2_ref import FLOOR, rel_err
from torcheasyrec_amd import _lib, personalized_net
from torcheasyrec_amd.personalized_net import EPNet, GateNU, PPNet

VEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_pepnet_vectors.npz"))
# as generated -- EPNet: (main, domain, hidden); PPNet: (main, uia, tasks, hidden units)
EP_CASES = {"ep_b9_m12_d4_h12": (12, 4, 12), "ep_b7_m20_d8_h8": (20, 8, 8)}
PP_CASES = {"pp_b9_m12_u8_t2_h8_4": (12, 8, 2, [8, 4]), "pp_b5_m16_u4_t3_h12": (16, 4, 3, [12])}
CASES = sorted(EP_CASES) + sorted(PP_CASES)


def ref_params(tag):
    return {k[len(tag) + len("/param/"):]: VEC[k] for k in VEC.files if k.startswith(f"{tag}/param/")}


def build(tag, dev):
    net = EPNet(*EP_CASES[tag], gamma=2.0) if tag in EP_CASES else PPNet(*PP_CASES[tag], gamma=2.0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in ref_params(tag).items()}, strict=True)
    return net.to(dev)


@pytest.fixture
def fwd_calls():
    """counts tzr_gate_scale_fwd calls of whichever library the test loaded"""
    calls = {"n": 0, "lib": None, "orig": None}

    def arm():
        L = _lib.lib()
        calls["lib"], calls["orig"] = L, L.tzr_gate_scale_fwd

        def counted(*a):
            calls["n"] += 1
            return calls["orig"](*a)

        L.tzr_gate_scale_fwd = counted
        return calls

    yield arm
    if calls["lib"] is not None:
        calls["lib"].tzr_gate_scale_fwd = calls["orig"]


@pytest.mark.parametrize("tag", CASES)
def test_state_dict_keys_are_the_references(tag):
    net = build(tag, torch.device("cpu"))
    assert set(net.state_dict()) == set(ref_params(tag))
    assert [n for n, _ in net.named_parameters()] == list(ref_params(tag))  # (and in the reference's order)
    if tag in PP_CASES:
        main, uia, T, hidden = PP_CASES[tag]
        assert net.output_dim() == [hidden[-1]] * T and net.task_output_dim() == hidden[-1]
        L = len(hidden)
        assert f"linears.{T * L - 1}.weight" in net.state_dict() and f"gate_nus.{T * L - 1}.dense_layers.2.bias" in net.state_dict()
        for t in range(T):
            for j in range(L):  # i = task * len(hidden_units) + layer
                assert net.linears[t * L + j].weight.shape == (hidden[j], hidden[j - 1] if j else main)
                assert net.gate_nus[t * L + j].dense_layers[0].weight.shape == (hidden[j], main + uia)
    else:
        assert sorted(net.state_dict()) == [f"gate_nu.dense_layers.{i}.{w}" for i in (0, 2) for w in ("bias", "weight")]
        assert net.output_dim() == EP_CASES[tag][0] and isinstance(net.gate_nu, GateNU)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", CASES)
def test_modules_reproduce_the_reference(dev, monkeypatch, fwd_calls, tag, fused):
    monkeypatch.setattr(personalized_net, "FUSED_GATE_SCALE", fused)
    calls = fwd_calls()
    net = build(tag, dev)
    x = torch.from_numpy(VEC[f"{tag}/x"]).to(dev).requires_grad_(True)
    side = torch.from_numpy(VEC[f"{tag}/side"]).to(dev).requires_grad_(True)
    ys = net(x, side)
    ys = list(ys) if isinstance(ys, (list, tuple)) else [ys]
    levels = len(PP_CASES[tag][3]) if tag in PP_CASES else 1
    assert calls["n"] == (levels if fused else 0)  # the fused path really is taken: one launch per PPNet level, one per EPNet
    gys = [torch.from_numpy(VEC[f"{tag}/gy{t}"]).to(dev) for t in range(len(ys))]
    torch.autograd.backward(ys, gys)
    got = {"y": ys, "gx": [x.grad, side.grad], "gparam": [p.grad for _, p in net.named_parameters()]}
    want = {"y": [VEC[f"{tag}/y{t}"] for t in range(len(ys))], "gx": [VEC[f"{tag}/gx"], VEC[f"{tag}/gside"]],
            "gparam": [VEC[f"{tag}/gparam/{k}"] for k in ref_params(tag)]}
    bad = []
    for kind in ("y", "gx", "gparam"):
        gap = float(VEC[f"ref_gap/{tag}/{kind}"])
        err, bound = rel_err(got[kind], [torch.from_numpy(w).double() for w in want[kind]]), max(4.0 * gap, FLOOR)
        print(f"{tag} fused={fused} {kind} on {dev.type}: err {err:.3e} ref_gap {gap:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("fused", [True, False])
def test_the_main_embedding_gets_no_gradient_through_the_gate(dev, monkeypatch, fused):
    """EPNet's gate reads main.detach(): whatever the gate's parameters are, d main = gamma * s * dout with s the gate's sigmoid,
    nothing more; the domain embedding does get a gradient.  PPNet's gates read main.detach() too: with every task's Linear
    layers zeroed nothing but the gates depends on main, and d main is exactly zero while d uia is not."""
    monkeypatch.setattr(personalized_net, "FUSED_GATE_SCALE", fused)
    tag = "ep_b9_m12_d4_h12"
    net = build(tag, dev)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(dev))
    x = torch.from_numpy(VEC[f"{tag}/x"]).to(dev).requires_grad_(True)
    side = torch.from_numpy(VEC[f"{tag}/side"]).to(dev).requires_grad_(True)
    gy = torch.from_numpy(VEC[f"{tag}/gy0"]).to(dev)
    net(x, side).backward(gy)
    with torch.no_grad():
        s = torch.sigmoid(net.gate_nu.dense_layers[:3](torch.cat([side, x], dim=-1)).double())
        want = 2.0 * s * gy.double()
    err = rel_err([x.grad], [want.cpu()])
    print(f"EPNet d main against gamma * s * dout on {dev.type} fused={fused}: {err:.3e}")
    assert err <= FLOOR and float(side.grad.abs().max()) > 0.0
    tag = "pp_b9_m12_u8_t2_h8_4"
    net = build(tag, dev)
    with torch.no_grad():
        for lin in net.linears:
            lin.weight.zero_()
            lin.bias.fill_(0.5)
    x = torch.from_numpy(VEC[f"{tag}/x"]).to(dev).requires_grad_(True)
    side = torch.from_numpy(VEC[f"{tag}/side"]).to(dev).requires_grad_(True)
    ys = net(x, side)
    torch.autograd.backward(ys, [torch.from_numpy(VEC[f"{tag}/gy{t}"]).to(dev) for t in range(len(ys))])
    assert float(x.grad.abs().max()) == 0.0 and float(side.grad.abs().max()) > 0.0


def test_shapes_the_kernel_refuses_take_the_literal_form(dev, fwd_calls):
    """a hidden width that is no multiple of 4, more than 8 tasks, another activation: gate_scale_ok (or the module) refuses,
    the literal form runs, nothing raises"""
    calls = fwd_calls()
    torch.manual_seed(0)
    x, side = torch.randn(6, 12, device=dev, requires_grad=True), torch.randn(6, 4, device=dev)
    for net in (PPNet(12, 4, 2, [6]), PPNet(12, 4, 9, [8]), PPNet(12, 4, 2, [8], activation="nn.Tanh"), EPNet(10, 4, 8)):
        net = net.to(dev)
        xin = x[:, :10] if isinstance(net, EPNet) else x
        ys = net(xin, side)
        ys = list(ys) if isinstance(ys, (list, tuple)) else [ys]
        sum(y.sum() for y in ys).backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    wide = PPNet(12, 4, 1, [4100]).to(dev)  # H = 4100: over the widest row
    sum(y.sum() for y in wide(x, side)).backward()
    empty = PPNet(12, 4, 2, [8]).to(dev)  # B = 0
    ys = empty(x[:0], side[:0])
    assert [tuple(y.shape) for y in ys] == [(0, 8)] * 2 and tuple(EPNet(12, 4, 8).to(dev)(x[:0], side[:0]).shape) == (0, 12)
    half = PPNet(12, 4, 2, [8]).to(dev).half()  # fp16
    ys = half(x.detach().half(), side.half())
    assert all(y.dtype == torch.float16 and bool(torch.isfinite(y).all()) for y in ys)
    assert calls["n"] == 0
    mixed = PPNet(12, 4, 2, [8, 6, 4]).to(dev)  # the middle level alone is refused
    sum(y.sum() for y in mixed(x, side)).backward()
    assert calls["n"] == 2
    # a main embedding whose rows the float4 accesses cannot take (a column slice at an odd offset) is copied, not refused
    ep = EPNet(12, 4, 8).to(dev)
    buf = torch.randn(6, 15, device=dev)
    got = ep(buf[:, 1:13], side)
    assert calls["n"] == 3
    torch.testing.assert_close(got, ep.gate_nu(torch.cat([side, buf[:, 1:13]], dim=-1)) * buf[:, 1:13], rtol=1e-5, atol=1e-6)
