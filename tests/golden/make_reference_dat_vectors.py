"""Generate tests/golden/reference_dat_vectors.npz by RUNNING the reference's own `tzrec.modules.mlp.MLP` and `nn.Linear`, wired
as the reference's DAT wires them (tzrec/models/dat.py:75-106: tower MLP over cat([input group, augment group]), output Linear,
F.normalize under COSINE, the augment rows handed back; dat.py:192-208: the similarity over the temperature and the detached tower
embeddings; match_model.py:50-64: the positive's multiply-and-sum, the negatives' matmul, the cat -- or the in-batch mm --;
match_model.py:281-336: CrossEntropyLoss against label 0 or arange(B), with sample weights mean(l w) / mean(w); dat.py:212-259: the
two Adaptive-Mimic terms, summed over everything or per row and then weighted the same way).

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_dat_vectors.py

`tzrec/modules/mlp.py` is imported from where it lies through the import shim of make_reference_module_vectors.py and executed
on CPU in fp32, with the modules' own initialisation; `dat.py` itself cannot be imported here (it pulls the dataset and protobuf
stack), so the wiring is this file's own words, as make_reference_dssm_vectors.py wires dssm.py by hand.

Per case: the towers' inputs `xu` [B, Du], `au` [B, D] and `xv` [M, Dv], `av` [M, D] (what their embedding groups would deliver for
the input and the augment group), the sample weights `w` (if any), every parameter `param/<key>` under the key the reference's DAT
gives it (`user_tower.mlp.mlp.<i>.perceptron.0.*`, `user_tower.output.*`, likewise `item_tower.*`), the scores `sim`, the losses
`loss` (softmax_cross_entropy), `amm_u`, `amm_i`, and the gradients `gxu`, `gau`, `gxv`, `gav`, `gparam/<key>` of the three losses'
sum.  `ref_gap/<case>/<kind>` (kind: sim, loss, gx, gparam) is the reference's own distance to a float64 evaluation of the same
modules on the same values, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: the yardstick the test scales its
bound with.  CASES is read by the test from here.
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

# case -> dict(B, N (sampled negatives; None: in-batch), Du, Dv, hidden, output_dim (= the augment groups' width), cosine,
# temperature, amm_u, amm_i, weights)
CASES = {
    "sampled_cos_b9_n12": dict(B=9, N=12, Du=24, Dv=25, hidden=[24, 16], output_dim=16, cosine=True, temperature=0.05, amm_u=0.5, amm_i=0.5,
                               weights=False),
    "inbatch_ip_b7_w": dict(B=7, N=None, Du=24, Dv=25, hidden=[24, 16], output_dim=16, cosine=False, temperature=1.0, amm_u=0.3, amm_i=1.3,
                            weights=True),
}
KINDS = ("sim", "loss", "gx", "gparam")


class Tower(nn.Module):
    """dat.py:75-80"""

    def __init__(self, MLP, d_in, d_aug, hidden, output_dim):
        super().__init__()
        self.mlp = MLP(d_in + d_aug, hidden_units=hidden)
        if output_dim > 0:
            self.output = nn.Linear(self.mlp.output_dim(), output_dim)


def tower_forward(t, x, a, cosine):
    """dat.py:93-104 in training mode"""
    out = t.mlp(torch.concat([x, a], dim=1))
    if hasattr(t, "output"):
        out = t.output(out)
    if cosine:
        out = F.normalize(out, p=2.0, dim=1)
    return out, a


def run(mod, c, xu, au, xv, av, w):
    leaves = [t.clone().requires_grad_(True) for t in (xu, au, xv, av)]
    xu, au, xv, av = leaves
    mod.zero_grad()
    user_tower_emb, user_augment = tower_forward(mod["user_tower"], xu, au, c["cosine"])
    item_tower_emb, item_augment = tower_forward(mod["item_tower"], xv, av, c["cosine"])
    B = user_tower_emb.shape[0]
    if c["N"] is None:  # match_model.py:50-52
        sim = torch.mm(user_tower_emb, item_tower_emb.T)
        label = torch.arange(B)
    else:  # match_model.py:54-64
        pos = torch.sum(user_tower_emb * item_tower_emb[:B], dim=-1, keepdim=True)
        neg = torch.matmul(user_tower_emb, item_tower_emb[B:].T)
        sim = torch.cat([pos, neg], dim=-1)
        label = torch.zeros(B, dtype=torch.long)
    sim = sim / c["temperature"]  # dat.py:192-199
    user_tower_emb, item_tower_emb = user_tower_emb.detach(), item_tower_emb.detach()  # dat.py:206-207
    if w is None:  # match_model.py:303-336
        loss = nn.CrossEntropyLoss()(sim, label)
    else:
        loss = torch.mean(nn.CrossEntropyLoss(reduction="none")(sim, label) * w) / torch.mean(w)
    batch_size = sim.size(0)  # dat.py:225-255
    dim = 1 if w is not None else (0, 1)
    amm_u = c["amm_u"] * torch.sum(torch.square(F.normalize(user_augment, p=2.0, dim=1) - item_tower_emb[:batch_size]), dim=dim)
    amm_i = c["amm_i"] * torch.sum(torch.square(F.normalize(item_augment[:batch_size], p=2.0, dim=1) - user_tower_emb), dim=dim)
    if w is not None:
        amm_u, amm_i = torch.mean(amm_u * w) / torch.mean(w), torch.mean(amm_i * w) / torch.mean(w)
    (loss + amm_u + amm_i).backward()
    return {"sim": [sim.detach()], "loss": [loss.detach(), amm_u.detach(), amm_i.detach()], "gx": [t.grad for t in leaves],
            "gparam": [p.grad.clone() for _, p in mod.named_parameters()]}


def main():
    from make_reference_module_vectors import _np, install_reference_imports

    install_reference_imports()
    MLP = importlib.import_module("tzrec.modules.mlp").MLP
    torch.manual_seed(20261021)
    torch.set_num_threads(1)
    out = {}
    for tag, c in CASES.items():
        D = c["output_dim"]
        mod = nn.ModuleDict({"user_tower": Tower(MLP, c["Du"], D, c["hidden"], D), "item_tower": Tower(MLP, c["Dv"], D, c["hidden"], D)})
        B, M = c["B"], c["B"] + (c["N"] or 0)
        xs = [torch.randn(B, c["Du"]), torch.randn(B, D), torch.randn(M, c["Dv"]), torch.randn(M, D)]
        w = 0.5 + torch.rand(B) if c["weights"] else None
        r32 = run(mod, c, *xs, w)
        r64 = run(copy.deepcopy(mod).double(), c, *[x.double() for x in xs], None if w is None else w.double())
        for name, x, g in zip(("xu", "au", "xv", "av"), xs, r32["gx"]):
            out[f"{tag}/{name}"], out[f"{tag}/g{name}"] = _np(x), _np(g)
        if w is not None:
            out[f"{tag}/w"] = _np(w)
        out[f"{tag}/sim"] = _np(r32["sim"][0])
        for name, l in zip(("loss", "amm_u", "amm_i"), r32["loss"]):
            out[f"{tag}/{name}"] = _np(l)
        for (n, p), g in zip(mod.named_parameters(), r32["gparam"]):
            out[f"{tag}/param/{n}"], out[f"{tag}/gparam/{n}"] = _np(p), _np(g)
        for kind in KINDS:
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_dat_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
