"""Generate tests/golden/reference_cross_vectors.npz by RUNNING the reference's own `Cross` module.

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_cross_vectors.py

`tzrec/modules/interaction.py:94-132` is imported from where it lies through the import shim of
make_reference_module_vectors.py and executed on CPU in fp32.  The reference initialises every bias to zero, which would
hide every bias term of the forward and of the weight gradient: the biases are set to random non-zero values first.

Per case (B, D, L): the input `x`, every `w<i>` [1, D] and `b<i>` [D], the output gradient `gy`, and the reference's `y`,
`gx`, `gw<i>`, `gb<i>`.  `ref_gap/<case>/<kind>` (kind: y, gx, gw, gb) is the reference's own distance to a float64
evaluation of the same module on the same values, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: the
yardstick the tests scale their bound with.
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

CASES = {"b6_d33_l3": (6, 33, 3), "b37_d429_l3": (37, 429, 3), "b9_d64_l1": (9, 64, 1)}


def _run(mod, x, gy):
    x = x.clone().requires_grad_(True)
    y = mod(x)
    y.backward(gy)
    return {"y": [y.detach()], "gx": [x.grad], "gw": [m.weight.grad for m in mod.w], "gb": [p.grad for p in mod.b]}


def main():
    install_reference_imports()
    ia_mod = importlib.import_module("tzrec.modules.interaction")
    torch.manual_seed(20261018)
    torch.set_num_threads(1)
    out = {}
    for tag, (B, D, L) in CASES.items():
        mod = ia_mod.Cross(D, L)
        with torch.no_grad():
            for p in mod.b:
                p.copy_(0.1 * torch.randn(D))
        x = 0.5 * torch.randn(B, D)
        gy = torch.randn(B, D)
        r32 = _run(mod, x, gy)
        r64 = _run(copy.deepcopy(mod).double(), x.double(), gy.double())
        out[f"{tag}/x"], out[f"{tag}/gy"] = _np(x), _np(gy)
        out[f"{tag}/y"], out[f"{tag}/gx"] = _np(r32["y"][0]), _np(r32["gx"][0])
        for i in range(L):
            out[f"{tag}/w{i}"], out[f"{tag}/b{i}"] = _np(mod.w[i].weight), _np(mod.b[i])
            out[f"{tag}/gw{i}"], out[f"{tag}/gb{i}"] = _np(r32["gw"][i]), _np(r32["gb"][i])
        for kind in ("y", "gx", "gw", "gb"):
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_cross_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
