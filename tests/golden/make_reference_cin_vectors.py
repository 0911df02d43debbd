"""Generate tests/golden/reference_cin_vectors.npz by RUNNING the reference's own `CIN` module.

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_cin_vectors.py

`tzrec/modules/interaction.py:183-233` is imported from where it lies through the import shim of
make_reference_module_vectors.py and executed on CPU in fp32 and, as a float64 deep copy, in float64.  Conv1d's default
biases are already non-zero; they are redrawn larger (0.1 N(0,1)) so that no bias term hides in the rounding.

Per case (B, F, D, layers): the input `x` [B, F, D], every `w<i>` [O_i, H_i F, 1] and `b<i>` [O_i], the output gradient `gy`,
and the reference's `y`, `gx`, `gw<i>`, `gb<i>`.  `ref_gap/<case>/<kind>` (kind: y, gx, gw, gb) is the reference's own distance
to the float64 evaluation on the same values, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: one of the two
yardsticks the tests scale their bound with (tests/cin_ref.py has the other).
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

CASES = {"b5_f3_d16": (5, 3, 16, [8, 4, 2]), "b37_f26_d16": (37, 26, 16, [32, 24]), "b9_f39_d8": (9, 39, 8, [20, 17, 1])}


def _run(mod, x, gy):
    x = x.clone().requires_grad_(True)
    y = mod(x)
    y.backward(gy)
    return {"y": [y.detach()], "gx": [x.grad], "gw": [m.weight.grad for m in mod.cin_layers], "gb": [m.bias.grad for m in mod.cin_layers]}


def main():
    install_reference_imports()
    ia_mod = importlib.import_module("tzrec.modules.interaction")
    torch.manual_seed(20261019)
    torch.set_num_threads(1)
    out = {}
    for tag, (B, F, D, layers) in CASES.items():
        mod = ia_mod.CIN(F, layers)
        with torch.no_grad():
            for m in mod.cin_layers:
                m.bias.copy_(0.1 * torch.randn(m.bias.shape))
        x = 0.5 * torch.randn(B, F, D)
        gy = torch.randn(B, sum(layers))
        r32 = _run(mod, x, gy)
        r64 = _run(copy.deepcopy(mod).double(), x.double(), gy.double())
        out[f"{tag}/x"], out[f"{tag}/gy"] = _np(x), _np(gy)
        out[f"{tag}/y"], out[f"{tag}/gx"] = _np(r32["y"][0]), _np(r32["gx"][0])
        for i, m in enumerate(mod.cin_layers):
            out[f"{tag}/w{i}"], out[f"{tag}/b{i}"] = _np(m.weight), _np(m.bias)
            out[f"{tag}/gw{i}"], out[f"{tag}/gb{i}"] = _np(r32["gw"][i]), _np(r32["gb"][i])
        for kind in ("y", "gx", "gw", "gb"):
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_cin_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
