"""Generate tests/golden/reference_dssm_vectors.npz by RUNNING the reference's own `tzrec.modules.mlp.MLP` and `nn.Linear`,
wired as the reference's DSSM wires them (tzrec/models/dssm.py:63-83: tower MLP, output Linear, F.normalize under COSINE;
match_model.py:50-64: the positive's multiply-and-sum, the negatives' matmul, the cat -- or the in-batch mm --; dssm.py:147-155:
the division by the temperature; match_model.py:281-336: CrossEntropyLoss against label 0 or arange(B), with sample weights
mean(l w) / mean(w)).

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_dssm_vectors.py

`tzrec/modules/mlp.py` is imported from where it lies through the import shim of make_reference_module_vectors.py and executed
on CPU in fp32, with the modules' own initialisation; `match_model.py` itself cannot be imported here (it pulls the dataset and
protobuf stack), so the wiring is this file's own words, as make_reference_module_vectors.py wires dlrm.py by hand.

Per case: the towers' inputs `xu` [B, Du] and `xv` [M, Dv] (what their embedding groups would deliver), the sample weights `w`
(if any), every parameter `param/<key>` under the key the reference's DSSM gives it (`user_tower.mlp.mlp.<i>.perceptron.0.*`,
`user_tower.output.*`, likewise `item_tower.*`), the scores `sim`, the `loss`, and the gradients `gxu`, `gxv`, `gparam/<key>` of
the loss.  `ref_gap/<case>/<kind>` (kind: sim, loss, gx, gparam) is the reference's own distance to a float64 evaluation of the
same modules on the same values, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: the yardstick the test scales
its bound with.  CASES is read by the test from here.
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# case -> dict(B, N (sampled negatives; None: in-batch), Du, Dv, hidden, output_dim, cosine, temperature, weights)
CASES = {
    "sampled_cos_b9_n12": dict(B=9, N=12, Du=24, Dv=25, hidden=[16, 8], output_dim=8, cosine=True, temperature=0.05, weights=False),
    "inbatch_ip_b7_w": dict(B=7, N=None, Du=24, Dv=25, hidden=[16, 8], output_dim=8, cosine=False, temperature=1.0, weights=True),
}
KINDS = ("sim", "loss", "gx", "gparam")


class Tower(nn.Module):
    """dssm.py:63-66"""

    def __init__(self, MLP, d_in, hidden, output_dim):
        super().__init__()
        self.mlp = MLP(d_in, hidden_units=hidden)
        if output_dim > 0:
            self.output = nn.Linear(self.mlp.output_dim(), output_dim)


def tower_forward(t, x, cosine):
    """dssm.py:77-83"""
    out = t.mlp(x)
    if hasattr(t, "output"):
        out = t.output(out)
    if cosine:
        out = F.normalize(out, p=2.0, dim=1)
    return out


def run(mod, c, xu, xv, w):
    xu, xv = xu.clone().requires_grad_(True), xv.clone().requires_grad_(True)
    mod.zero_grad()
    u, v = tower_forward(mod["user_tower"], xu, c["cosine"]), tower_forward(mod["item_tower"], xv, c["cosine"])
    B = u.shape[0]
    if c["N"] is None:  # match_model.py:50-52
        sim = torch.mm(u, v.T)
        label = torch.arange(B)
    else:  # match_model.py:54-64
        pos = torch.sum(u * v[:B], dim=-1, keepdim=True)
        neg = torch.matmul(u, v[B:].T)
        sim = torch.cat([pos, neg], dim=-1)
        label = torch.zeros(B, dtype=torch.long)
    sim = sim / c["temperature"]  # dssm.py:147-155
    if w is None:  # match_model.py:303-336
        loss = nn.CrossEntropyLoss()(sim, label)
    else:
        loss = torch.mean(nn.CrossEntropyLoss(reduction="none")(sim, label) * w) / torch.mean(w)
    loss.backward()
    return {"sim": [sim.detach()], "loss": [loss.detach()], "gx": [xu.grad, xv.grad], "gparam": [p.grad.clone() for _, p in mod.named_parameters()]}


def main():
    from make_reference_module_vectors import _np, install_reference_imports

    install_reference_imports()
    MLP = importlib.import_module("tzrec.modules.mlp").MLP
    torch.manual_seed(20261020)
    torch.set_num_threads(1)
    out = {}
    for tag, c in CASES.items():
        mod = nn.ModuleDict({"user_tower": Tower(MLP, c["Du"], c["hidden"], c["output_dim"]),
                             "item_tower": Tower(MLP, c["Dv"], c["hidden"], c["output_dim"])})
        B, M = c["B"], c["B"] + (c["N"] or 0)
        xu, xv = torch.randn(B, c["Du"]), torch.randn(M, c["Dv"])
        w = 0.5 + torch.rand(B) if c["weights"] else None
        r32 = run(mod, c, xu, xv, w)
        r64 = run(copy.deepcopy(mod).double(), c, xu.double(), xv.double(), None if w is None else w.double())
        out[f"{tag}/xu"], out[f"{tag}/xv"] = _np(xu), _np(xv)
        if w is not None:
            out[f"{tag}/w"] = _np(w)
        out[f"{tag}/sim"], out[f"{tag}/loss"] = _np(r32["sim"][0]), _np(r32["loss"][0])
        out[f"{tag}/gxu"], out[f"{tag}/gxv"] = _np(r32["gx"][0]), _np(r32["gx"][1])
        for (n, p), g in zip(mod.named_parameters(), r32["gparam"]):
            out[f"{tag}/param/{n}"], out[f"{tag}/gparam/{n}"] = _np(p), _np(g)
        for kind in KINDS:
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_dssm_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
