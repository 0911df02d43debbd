"""Generate tests/golden/reference_dbmtl_vectors.npz by RUNNING the reference's own `tzrec.modules.mlp.MLP` and `nn.Linear`,
wired as `DBMTL.predict` wires them (tzrec/models/dbmtl.py:147-173: the towers' MLPs, the relation MLPs over the concatenation
of the tower's own output with the relation outputs of the towers it names, the logits layers).

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_dbmtl_vectors.py

`tzrec/modules/mlp.py` is imported from where it lies through the import shim of make_reference_module_vectors.py and executed
on CPU in fp32, with the modules' own initialisation.  Every tower reads the one input `x` (the model without MMoE).

Per case: `x`, every parameter `param/<key>` under the key the reference's DBMTL gives it (`task_mlps.<tower>.mlp.<i>.
perceptron.0.*`, `relation_mlps.<tower>...`, `task_outputs.<i>.*`), the logit gradients `gy<i>`, and the reference's logits
`y<i>`, input gradient `gx` and parameter gradients `gparam/<key>`.  `ref_gap/<case>/<kind>` (kind: y, gx, gparam) is the
reference's own distance to a float64 evaluation of the same modules on the same values, max |fp32 - fp64| / max(1, |fp64|) over
the tensors of the kind: the yardstick the test scales its bound with.  The towers of a case are `TOWERS` below, which the test
reads from here: (tower name, mlp hidden units or None, relation tower names, relation_mlp hidden units or None).
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# case -> (B, input width, towers)
CASES = {
    "chain_b9_in12": (9, 12, [("ctr", [8], [], None), ("cvr", [8, 12], ["ctr"], [16, 8]), ("pay", [8], ["ctr", "cvr"], [12])]),
    "bare_b7_in16": (7, 16, [("a", None, [], None), ("b", None, ["a"], [8]), ("c", [4], ["b", "a"], [12, 4]), ("d", [8], ["c"], None)]),
}
KINDS = ("y", "gx", "gparam")


def build(MLP, d_in, towers):
    """the three containers of dbmtl.py:84-123"""
    task_mlps, relation_mlps, task_outputs = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleList()
    for name, hidden, _, _ in towers:
        if hidden is not None:
            task_mlps[name] = MLP(d_in, hidden_units=hidden)
    for name, _, rel, rel_hidden in towers:
        if rel_hidden is not None:
            d = task_mlps[name].output_dim() if name in task_mlps else d_in
            for r in rel:
                d += relation_mlps[r].output_dim() if r in relation_mlps else (task_mlps[r].output_dim() if r in task_mlps else d_in)
            relation_mlps[name] = MLP(d, hidden_units=rel_hidden)
    for name, _, _, _ in towers:
        d = relation_mlps[name].output_dim() if name in relation_mlps else (task_mlps[name].output_dim() if name in task_mlps else d_in)
        task_outputs.append(nn.Linear(d, 1))
    return nn.ModuleDict({"task_mlps": task_mlps, "relation_mlps": relation_mlps, "task_outputs": task_outputs})


def run(mod, towers, x, gys):
    """dbmtl.py:147-173"""
    x = x.clone().requires_grad_(True)
    mod.zero_grad()
    task_net = {name: mod["task_mlps"][name](x) if name in mod["task_mlps"] else x for name, _, _, _ in towers}
    relation_net = {}
    for name, _, rel, rel_hidden in towers:
        if rel_hidden is not None:
            relation_net[name] = mod["relation_mlps"][name](torch.cat([task_net[name]] + [relation_net[r] for r in rel], dim=1))
        else:
            relation_net[name] = task_net[name]
    ys = [mod["task_outputs"][i](relation_net[name]) for i, (name, _, _, _) in enumerate(towers)]
    torch.autograd.backward(ys, gys)
    return {"y": [y.detach() for y in ys], "gx": [x.grad], "gparam": [p.grad.clone() for _, p in mod.named_parameters()]}


def main():
    from make_reference_module_vectors import _np, install_reference_imports

    install_reference_imports()
    MLP = importlib.import_module("tzrec.modules.mlp").MLP
    torch.manual_seed(20261020)
    torch.set_num_threads(1)
    out = {}
    for tag, (B, d_in, towers) in CASES.items():
        mod = build(MLP, d_in, towers)
        x = torch.randn(B, d_in)
        gys = [torch.randn(B, 1) for _ in towers]
        r32 = run(mod, towers, x, gys)
        r64 = run(copy.deepcopy(mod).double(), towers, x.double(), [g.double() for g in gys])
        out[f"{tag}/x"], out[f"{tag}/gx"] = _np(x), _np(r32["gx"][0])
        for i, (gy, y) in enumerate(zip(gys, r32["y"])):
            out[f"{tag}/gy{i}"], out[f"{tag}/y{i}"] = _np(gy), _np(y)
        for (n, p), g in zip(mod.named_parameters(), r32["gparam"]):
            out[f"{tag}/param/{n}"], out[f"{tag}/gparam/{n}"] = _np(p), _np(g)
        for kind in KINDS:
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_dbmtl_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
