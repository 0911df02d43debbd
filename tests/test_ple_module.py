"""ple.ExtractionNet (one CGC level of PLE) against vectors recorded from the reference's own module
(tests/golden/make_reference_ple_vectors.py running tzrec/modules/extraction_net.py): loaded with the reference's parameters
under the reference's state-dict keys it reproduces the reference's outputs, input gradients and parameter gradients, with the
gate-and-mix step fused (gate_ops.cgc_mix, one tzr_cgc_mix_fwd per level) and in the literal form.  Bound per kind: 4 x the
reference's own fp32-vs-float64 distance stored with the vectors (the factor tests/test_cross_v2.py and tests/test_wukong_module.py
hold their modules to against the same yardstick), floor 2^-20 as there."""
import os
import re

import numpy as np
import pytest
import torch

from cross_v2_ref import FLOOR, rel_err
from torcheasyrec_amd import _lib, ple
from torcheasyrec_amd.ple import ExtractionNet

VEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_ple_vectors.npz"))
# case: (task input widths, shared input width, share_num, expert_num_per_task, share hidden, task hidden, final_flag) -- as generated
CASES = {
    "first_t2_p2_s1": ([13, 13], 13, 1, 2, [8], [12, 8], False),
    "last_t2_p1_s2": ([8, 12], 20, 2, 1, [10, 16], [16], True),
    "mid_t3_p2_s2": ([8, 12, 4], 8, 2, 2, [12], [6, 12], False),
}


def our_key(ref_key: str) -> str:
    """the package's MLP keeps Linear i of a plain stack at `mlp.<2i>` (Linear, ReLU, Linear, ...), the reference at
    `mlp.<i>.perceptron.0`"""
    return re.sub(r"mlp\.(\d+)\.perceptron\.0\.", lambda m: f"mlp.{2 * int(m.group(1))}.", ref_key)


def ref_params(tag):
    return {k[len(tag) + len("/param/"):]: VEC[k] for k in VEC.files if k.startswith(f"{tag}/param/")}


def build(tag, dev):
    d_task, d_shared, S, P, share_h, task_h, final = CASES[tag]
    net = ExtractionNet(d_task, d_shared, tag, S, P, {"hidden_units": share_h}, {"hidden_units": task_h}, final_flag=final)
    net.load_state_dict({our_key(k): torch.from_numpy(v) for k, v in ref_params(tag).items()}, strict=True)
    return net.to(dev)


@pytest.fixture
def fwd_calls():
    """counts tzr_cgc_mix_fwd calls of whichever library the test loaded"""
    calls = {"n": 0, "lib": None, "orig": None}

    def arm():
        L = _lib.lib()
        calls["lib"], calls["orig"] = L, L.tzr_cgc_mix_fwd

        def counted(*a):
            calls["n"] += 1
            return calls["orig"](*a)

        L.tzr_cgc_mix_fwd = counted
        return calls

    yield arm
    if calls["lib"] is not None:
        calls["lib"].tzr_cgc_mix_fwd = calls["orig"]


@pytest.mark.parametrize("tag", sorted(CASES))
def test_state_dict_keys_are_the_references(tag):
    net = build(tag, torch.device("cpu"))
    assert set(net.state_dict()) == {our_key(k) for k in ref_params(tag)}
    assert [n for n, _ in net.named_parameters()] == [our_key(k) for k in ref_params(tag)]  # (and in the reference's order)
    assert net.output_dim() == [CASES[tag][5][-1]] * len(CASES[tag][0]) + [CASES[tag][4][-1]]
    assert (net._shared_gate is None) == CASES[tag][6]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_extraction_net_reproduces_the_reference(dev, monkeypatch, fwd_calls, tag, fused):
    monkeypatch.setattr(ple, "FUSED_CGC_MIX", fused)
    calls = fwd_calls()
    T, final = len(CASES[tag][0]), CASES[tag][6]
    net = build(tag, dev)
    xs = [torch.from_numpy(VEC[f"{tag}/x{t}"]).to(dev).requires_grad_(True) for t in range(T)]
    x_shared = torch.from_numpy(VEC[f"{tag}/xs"]).to(dev).requires_grad_(True)
    outs, shared = net(xs, x_shared)
    assert calls["n"] == (1 if fused else 0)  # the fused path really is taken: one launch for the level
    assert len(outs) == T and (shared is None) == final
    ys = list(outs) + ([] if final else [shared])
    gys = [torch.from_numpy(VEC[f"{tag}/gy{t}"]).to(dev) for t in range(T)] + ([] if final else [torch.from_numpy(VEC[f"{tag}/gys"]).to(dev)])
    torch.autograd.backward(ys, gys)
    names = [f"y{t}" for t in range(T)] + ([] if final else ["ys"])
    got = {"y": ys, "gx": [x.grad for x in xs] + [x_shared.grad], "gparam": [p.grad for _, p in net.named_parameters()]}
    want = {"y": [VEC[f"{tag}/{n}"] for n in names], "gx": [VEC[f"{tag}/gx{t}"] for t in range(T)] + [VEC[f"{tag}/gxs"]],
            "gparam": [VEC[f"{tag}/gparam/{k}"] for k in ref_params(tag)]}
    bad = []
    for kind in ("y", "gx", "gparam"):
        gap = float(VEC[f"ref_gap/{tag}/{kind}"])
        err, bound = rel_err(got[kind], [torch.from_numpy(w).double() for w in want[kind]]), max(4.0 * gap, FLOOR)
        print(f"{tag} fused={fused} {kind} on {dev.type}: err {err:.3e} ref_gap {gap:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, bad
