"""Generate tests/golden/reference_cross_v2_vectors.npz by RUNNING the reference's own `CrossV2` module.

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_cross_v2_vectors.py

`tzrec/modules/interaction.py:135-180` is imported from where it lies through the import shim of
make_reference_module_vectors.py and executed on CPU in fp32, with the module's own initialisation (nn.Linear's default:
weights and biases non-zero).

Per case (B, D, r, L): the input `x`, every `u<i>` [r, D], `v<i>` [D, r] and `c<i>` [D] (`u_kernels.<i>.weight`,
`v_kernels.<i>.weight`, `v_kernels.<i>.bias`), the output gradient `gy`, and the reference's `y`, `gx`, `gu<i>`, `gv<i>`,
`gc<i>`.  `ref_gap/<case>/<kind>` (kind: y, gx, gu, gv, gc) is the reference's own distance to a float64 evaluation of the
same module on the same values, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: the yardstick the tests
scale their bound with.
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

CASES = {"b6_d33_r3_l3": (6, 33, 3, 3), "b21_d429_r32_l2": (21, 429, 32, 2), "b9_d64_r16_l1": (9, 64, 16, 1)}
KINDS = ("y", "gx", "gu", "gv", "gc")


def _run(mod, x, gy):
    x = x.clone().requires_grad_(True)
    y = mod(x)
    y.backward(gy)
    return {"y": [y.detach()], "gx": [x.grad], "gu": [m.weight.grad for m in mod.u_kernels], "gv": [m.weight.grad for m in mod.v_kernels],
            "gc": [m.bias.grad for m in mod.v_kernels]}


def main():
    install_reference_imports()
    ia_mod = importlib.import_module("tzrec.modules.interaction")
    torch.manual_seed(20261019)
    torch.set_num_threads(1)
    out = {}
    for tag, (B, D, R, L) in CASES.items():
        mod = ia_mod.CrossV2(D, L, R)
        x = 0.5 * torch.randn(B, D)
        gy = torch.randn(B, D)
        r32 = _run(mod, x, gy)
        r64 = _run(copy.deepcopy(mod).double(), x.double(), gy.double())
        out[f"{tag}/x"], out[f"{tag}/gy"] = _np(x), _np(gy)
        out[f"{tag}/y"], out[f"{tag}/gx"] = _np(r32["y"][0]), _np(r32["gx"][0])
        for i in range(L):
            out[f"{tag}/u{i}"], out[f"{tag}/v{i}"] = _np(mod.u_kernels[i].weight), _np(mod.v_kernels[i].weight)
            out[f"{tag}/c{i}"] = _np(mod.v_kernels[i].bias)
            out[f"{tag}/gu{i}"], out[f"{tag}/gv{i}"], out[f"{tag}/gc{i}"] = _np(r32["gu"][i]), _np(r32["gv"][i]), _np(r32["gc"][i])
        for kind in KINDS:
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_cross_v2_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
