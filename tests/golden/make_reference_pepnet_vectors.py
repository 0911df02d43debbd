"""Generate tests/golden/reference_pepnet_vectors.npz by RUNNING the reference's own `EPNet` and `PPNet` modules.

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_pepnet_vectors.py

`tzrec/modules/personalized_net.py` is imported from where it lies through the import shim of
make_reference_module_vectors.py and executed on CPU in fp32, with the modules' own initialisation.

Per case: the main input `x` and the gate's side input `side` (EPNet: the domain embedding, PPNet: the uia embedding), every
parameter `param/<state-dict key>` under the reference's own key, the output gradients `gy<t>` (EPNet: `gy0`), and the
reference's outputs `y<t>`, input gradients `gx` / `gside` and parameter gradients `gparam/<key>`.  `ref_gap/<case>/<kind>`
(kind: y, gx, gparam) is the reference's own distance to a float64 evaluation of the same module on the same values,
max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: the yardstick the tests scale their bound with.
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

# EPNet: (B, main, domain, hidden);  PPNet: (B, main, uia, tasks, hidden units)
EP_CASES = {"ep_b9_m12_d4_h12": (9, 12, 4, 12), "ep_b7_m20_d8_h8": (7, 20, 8, 8)}
PP_CASES = {"pp_b9_m12_u8_t2_h8_4": (9, 12, 8, 2, [8, 4]), "pp_b5_m16_u4_t3_h12": (5, 16, 4, 3, [12])}
KINDS = ("y", "gx", "gparam")


def _run(mod, x, side, gys):
    x, side = x.clone().requires_grad_(True), side.clone().requires_grad_(True)
    mod.zero_grad()
    ys = mod(x, side)
    ys = list(ys) if isinstance(ys, (list, tuple)) else [ys]
    torch.autograd.backward(ys, gys)
    return {"y": [y.detach() for y in ys], "gx": [x.grad, side.grad], "gparam": [p.grad.clone() for _, p in mod.named_parameters()]}


def main():
    install_reference_imports()
    mod_py = importlib.import_module("tzrec.modules.personalized_net")
    torch.manual_seed(20261020)
    torch.set_num_threads(1)
    out = {}
    cases = [(tag, mod_py.EPNet(m, d, h, gamma=2.0), B, m, d, [m]) for tag, (B, m, d, h) in EP_CASES.items()]
    cases += [(tag, mod_py.PPNet(m, u, T, hidden, gamma=2.0), B, m, u, [hidden[-1]] * T) for tag, (B, m, u, T, hidden) in PP_CASES.items()]
    for tag, mod, B, d_main, d_side, d_outs in cases:
        x, side = 0.5 * torch.randn(B, d_main), 0.5 * torch.randn(B, d_side)
        gys = [torch.randn(B, d) for d in d_outs]
        r32 = _run(mod, x, side, gys)
        r64 = _run(copy.deepcopy(mod).double(), x.double(), side.double(), [g.double() for g in gys])
        out[f"{tag}/x"], out[f"{tag}/side"] = _np(x), _np(side)
        out[f"{tag}/gx"], out[f"{tag}/gside"] = _np(r32["gx"][0]), _np(r32["gx"][1])
        for t, (gy, y) in enumerate(zip(gys, r32["y"])):
            out[f"{tag}/gy{t}"], out[f"{tag}/y{t}"] = _np(gy), _np(y)
        for (n, p), g in zip(mod.named_parameters(), r32["gparam"]):
            out[f"{tag}/param/{n}"], out[f"{tag}/gparam/{n}"] = _np(p), _np(g)
        assert sorted(n for n, _ in mod.named_parameters()) == sorted(mod.state_dict())
        for kind in KINDS:
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_pepnet_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
