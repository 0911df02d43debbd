"""Generate tests/golden/reference_ple_vectors.npz by RUNNING the reference's own `ExtractionNet` module (one CGC level of PLE).

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_ple_vectors.py

`tzrec/modules/extraction_net.py:20-139` is imported from where it lies through the import shim of
make_reference_module_vectors.py and executed on CPU in fp32, with the module's own initialisation.

Per case: the task inputs `x<t>` and the shared input `xs`, every parameter `param/<state-dict key>` under the reference's own
key, the output gradients `gy<t>` (and `gys` on a level that has a shared gate), and the reference's outputs `y<t>` / `ys`,
input gradients `gx<t>` / `gxs` and parameter gradients `gparam/<key>`.  `ref_gap/<case>/<kind>` (kind: y, gx, gparam) is the
reference's own distance to a float64 evaluation of the same module on the same values, max |fp32 - fp64| / max(1, |fp64|)
over the tensors of the kind: the yardstick the tests scale their bound with.
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

# case: (B, task input widths, shared input width, share_num, expert_num_per_task, share hidden, task hidden, final_flag)
CASES = {
    "first_t2_p2_s1": (9, [13, 13], 13, 1, 2, [8], [12, 8], False),
    "last_t2_p1_s2": (7, [8, 12], 20, 2, 1, [10, 16], [16], True),  # a later level: unequal task input widths, no shared gate
    "mid_t3_p2_s2": (5, [8, 12, 4], 8, 2, 2, [12], [6, 12], False),
}
KINDS = ("y", "gx", "gparam")


def _run(mod, xs_task, x_shared, gys):
    xs_task = [x.clone().requires_grad_(True) for x in xs_task]
    x_shared = x_shared.clone().requires_grad_(True)
    mod.zero_grad()
    outs, shared = mod(xs_task, x_shared)
    ys = list(outs) + ([shared] if shared is not None else [])
    torch.autograd.backward(ys, gys[:len(ys)])
    return {"y": [y.detach() for y in ys], "gx": [x.grad for x in xs_task] + [x_shared.grad],
            "gparam": [p.grad.clone() for _, p in mod.named_parameters()]}


def main():
    install_reference_imports()
    mod_py = importlib.import_module("tzrec.modules.extraction_net")
    torch.manual_seed(20261019)
    torch.set_num_threads(1)
    out = {}
    for tag, (B, d_task, d_shared, S, P, share_h, task_h, final) in CASES.items():
        mod = mod_py.ExtractionNet(d_task, d_shared, tag, S, P, {"hidden_units": share_h}, {"hidden_units": task_h}, final_flag=final)
        T = len(d_task)
        xs_task, x_shared = [0.5 * torch.randn(B, d) for d in d_task], 0.5 * torch.randn(B, d_shared)
        gys = [torch.randn(B, task_h[-1]) for _ in range(T)] + [torch.randn(B, share_h[-1])]
        r32 = _run(mod, xs_task, x_shared, gys)
        r64 = _run(copy.deepcopy(mod).double(), [x.double() for x in xs_task], x_shared.double(), [g.double() for g in gys])
        names = [n for n, _ in mod.named_parameters()]
        for t in range(T):
            out[f"{tag}/x{t}"], out[f"{tag}/gy{t}"] = _np(xs_task[t]), _np(gys[t])
            out[f"{tag}/y{t}"], out[f"{tag}/gx{t}"] = _np(r32["y"][t]), _np(r32["gx"][t])
        out[f"{tag}/xs"], out[f"{tag}/gxs"] = _np(x_shared), _np(r32["gx"][T])
        if not final:
            out[f"{tag}/gys"], out[f"{tag}/ys"] = _np(gys[T]), _np(r32["y"][T])
        for (n, p), g in zip(mod.named_parameters(), r32["gparam"]):
            out[f"{tag}/param/{n}"], out[f"{tag}/gparam/{n}"] = _np(p), _np(g)
        assert sorted(names) == sorted(mod.state_dict())
        for kind in KINDS:
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_ple_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
