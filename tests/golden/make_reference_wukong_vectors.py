"""Generate tests/golden/reference_wukong_vectors.npz by RUNNING the reference's own `WuKongLayer`.

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_wukong_vectors.py

`tzrec/modules/interaction.py:236-378` is imported from where it lies through the import shim of make_reference_module_vectors.py
and executed on CPU in fp32.  The reference initialises every LayerNorm to weight 1 and bias 0, which would hide gamma and
beta: they are set to random values first.

Per case (B, F, D, Fl, Ff, k, mlp): the input `x`, every parameter `p:<state-dict key>`, the output gradient `gy`, and the
reference's `y`, `gx`, `g:<state-dict key>`.  `ref_gap/<case>/<kind>` is the reference's own distance to a float64 evaluation of
the same module on the same values, max |fp32 - fp64| / max(1, |fp64|): the yardstick the tests scale their bound with.  Kinds:
y, gx, and one per parameter (`g:lcb.weight`, `g:residual_projection.weight`, ...).  `keys/<case>` is the reference's list of
state-dict keys.

No case may hold a ReLU pre-activation of the FMB's MLP within 2^-16 of zero in float64 (the fp32 run could take the other side
there): the script asserts it and moves on to the next seed otherwise.
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

# (B, F, D, Fl, Ff, k, mlp): the reference test's first layer (a projection residual), an identity residual, the example's
# first layer with a narrow MLP
CASES = {"b6_f3_d8_l3_f4_k2": (6, 3, 8, 3, 4, 2, [4]), "b6_f7_d8_l3_f4_k3": (6, 7, 8, 3, 4, 3, [4]),
         "b9_f27_d128_l16_f16_k24": (9, 27, 128, 16, 16, 24, [16])}
KINK = 2.0 ** -16


def _run(mod, x, gy):
    """forward + backward; the pre-activations of every ReLU are collected by hooks on the nn.ReLU modules"""
    pre = []
    hooks = [m.register_forward_hook(lambda _m, inp, _out: pre.append(inp[0].detach())) for m in mod.modules()
             if isinstance(m, torch.nn.ReLU)]
    mod.zero_grad()
    x = x.clone().requires_grad_(True)
    y = mod(x)
    y.backward(gy)
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), "gx": x.grad}
    out.update({f"g:{k}": p.grad for k, p in mod.named_parameters()})
    return out, pre


def _case(ia_mod, B, F, D, Fl, Ff, k, mlp, seed):
    torch.manual_seed(seed)
    mod = ia_mod.WuKongLayer(D, F, Fl, Ff, k, {"hidden_units": mlp})
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape))
    x = torch.randn(B, F, D)
    gy = torch.randn(B, mod.output_feature_num(), D)
    r32, _ = _run(mod, x, gy)
    r64, pre = _run(copy.deepcopy(mod).double(), x.double(), gy.double())
    assert pre, "no ReLU was seen: the hooks missed the FMB's MLP"
    if any(bool((p.abs() < KINK).any()) for p in pre):
        return None
    return mod, x, gy, r32, r64


def main():
    install_reference_imports()
    ia_mod = importlib.import_module("tzrec.modules.interaction")
    torch.set_num_threads(1)
    out = {}
    for tag, (B, F, D, Fl, Ff, k, mlp) in CASES.items():
        seed = 20261019
        while (res := _case(ia_mod, B, F, D, Fl, Ff, k, mlp, seed)) is None:
            seed += 1
        mod, x, gy, r32, r64 = res
        assert not any(bool((p.abs() < KINK).any()) for p in _run(copy.deepcopy(mod).double(), x.double(), gy.double())[1])
        assert ("residual_projection.weight" in mod.state_dict()) == (F != Fl + Ff)
        out[f"{tag}/x"], out[f"{tag}/gy"] = _np(x), _np(gy)
        out[f"keys/{tag}"] = np.array(list(mod.state_dict()))
        for key, p in mod.state_dict().items():
            out[f"{tag}/p:{key}"] = _np(p)
        for name in r32:
            out[f"{tag}/{name}"] = _np(r32[name])
            a, e = r32[name].double(), r64[name]
            out[f"ref_gap/{tag}/{name}"] = np.float64(float(((a - e).abs() / e.abs().clamp(min=1.0)).max()))
        print(tag, "seed", seed, {n: f"{float(out[f'ref_gap/{tag}/{n}']):.2e}" for n in ("y", "gx", "g:lcb.weight", "g:fmb.weight")})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_wukong_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
