"""Generate tests/golden/reference_mind_vectors.npz by RUNNING the reference's own `tzrec.modules.capsule.CapsuleLayer` (its
config a plain namespace), `tzrec.modules.mlp.MLP` and `nn.Linear`, wired as the reference's MIND wires them (tzrec/models/
mind.py:67-141: user_mlp / user_mlp_out, _hist_seq_mlp / _hist_seq_mlp_out without bias, _capsule_layer, _concat_mlp, output
without bias; mind.py:154-194: the user tower's forward; mind.py:244-252: the item tower's; mind.py:303-333: label-aware
attention; match_model.py:54-64: the positive's multiply-and-sum, the negatives' matmul, the cat; mind.py:359-364: the division by
the temperature; match_model.py:303-336: CrossEntropyLoss against label 0).

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_mind_vectors.py

The modules are imported from where they lie through the import shim of make_reference_module_vectors.py and executed on CPU in
fp32 with their own initialisation; `mind.py` itself cannot be imported here (it pulls the dataset and protobuf stack), so the
wiring is this file's own words.

Per case (B = 6 histories of 0, 1, 3, 4, 9 and 25 clicks at max_seq_len 20, 5 sampled negatives): the user group's features `xu`
[B, Du], the history padded as the reference's embedding group delivers it `hist` [B, 25, Dh] with `lengths`, the item rows `xv`
[M, Dv], for `normal` init the drawn routing logits `logits0` [B, S, K] (recorded by re-seeding the generator the layer drew
from), every parameter `param/<key>` under the key the reference's MIND gives it, `high` [B, K, H] and `mask` out of the capsule
layer, `sim`, `loss`, and the gradients `gxu`, `ghist`, `gxv`, `gparam/<key>` of the loss.  `ref_gap/<case>/<kind>` (kind: high,
sim, loss, gx, gparam) is the reference's own distance to a float64 evaluation of the same modules on the same values and the same
drawn logits, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind.  CASES is read by the test from here.
"""
import copy
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LENGTHS = [0, 1, 3, 4, 9, 25]
BASE = dict(Du=24, Dh=24, Dv=25, user_mlp=[16, 8], hist_seq_mlp=[16, 12], concat_mlp=[16, 8], item_mlp=[16, 8], output_dim=8, N=5,
            max_k=3, max_seq_len=20, high_dim=8, num_iters=3, simi_pow=10.0, temperature=0.05)
CASES = {
    "zeros": dict(BASE, routing_init_method="zeros", routing_logits_scale=20.0, routing_logits_stddev=1.0, squash_pow=1.0),
    "normal": dict(BASE, routing_init_method="normal", routing_logits_scale=1.0, routing_logits_stddev=0.1, squash_pow=2.0),
}
KINDS = ("high", "sim", "loss", "gx", "gparam")
DRAW_SEED = 77


def capsule_namespace(c):
    return SimpleNamespace(max_seq_len=c["max_seq_len"], max_k=c["max_k"], high_dim=c["high_dim"], num_iters=c["num_iters"],
                           routing_logits_scale=c["routing_logits_scale"], routing_logits_stddev=c["routing_logits_stddev"],
                           squash_pow=c["squash_pow"], const_caps_num=False, routing_init_method=c["routing_init_method"])


class UserTower(nn.Module):
    """mind.py:67-141"""

    def __init__(self, MLP, CapsuleLayer, c):
        super().__init__()
        self.user_mlp = MLP(in_features=c["Du"], hidden_units=c["user_mlp"][0:-1], activation="nn.ReLU", use_bn=False, dropout_ratio=None)
        self.user_mlp_out = nn.Linear(self.user_mlp.output_dim(), c["user_mlp"][-1])
        self._hist_seq_mlp = MLP(in_features=c["Dh"], dim=3, hidden_units=c["hist_seq_mlp"][0:-1], activation="nn.ReLU", use_bn=False, bias=False,
                                 dropout_ratio=None)
        self._hist_seq_mlp_out = nn.Linear(self._hist_seq_mlp.output_dim(), c["hist_seq_mlp"][-1], bias=False)
        self._capsule_layer = CapsuleLayer(capsule_config=capsule_namespace(c), input_dim=c["hist_seq_mlp"][-1])
        self._concat_mlp = MLP(in_features=c["user_mlp"][-1] + c["high_dim"], dim=3, hidden_units=c["concat_mlp"])
        self.output = nn.Linear(self._concat_mlp.output_dim(), c["output_dim"], bias=False)


class ItemTower(nn.Module):
    """mind.py:229-232"""

    def __init__(self, MLP, c):
        super().__init__()
        self.mlp = MLP(c["Dv"], hidden_units=c["item_mlp"])
        self.output = nn.Linear(self.mlp.output_dim(), c["output_dim"])


def run(mod, c, xu, hist, lengths, xv):
    xu, hist, xv = xu.clone().requires_grad_(True), hist.clone().requires_grad_(True), xv.clone().requires_grad_(True)
    mod.zero_grad()
    ut, it = mod["user_tower"], mod["item_tower"]
    user_feature = ut.user_mlp_out(ut.user_mlp(xu))  # mind.py:158-161
    hist_seq_feas = ut._hist_seq_mlp_out(ut._hist_seq_mlp(hist))  # mind.py:165-167
    torch.manual_seed(DRAW_SEED)  # (the layer draws its `normal` logits from the global generator)
    high, mask = ut._capsule_layer(hist_seq_feas, lengths)
    high.retain_grad()
    user_feature = torch.unsqueeze(user_feature, dim=1)  # mind.py:178-189
    tile = torch.tile(user_feature, [1, high.shape[1], 1])
    interests = torch.cat([tile, high], dim=-1)
    interests = interests * mask.unsqueeze(-1).float().to(interests.dtype)
    interests = ut._concat_mlp(interests)
    interests = interests * mask.unsqueeze(-1).float().to(interests.dtype)
    interests = ut.output(interests)
    interests = F.normalize(interests, p=2.0, dim=-1)
    item_emb = F.normalize(it.output(it.mlp(xv)), p=2.0, dim=1)  # mind.py:244-252
    B = interests.size(0)  # mind.py:319-333
    weight = torch.einsum("bkd, bd->bk", interests, item_emb[:B])
    threshold = (mask.float().to(weight.dtype) * 2 - 1) * float("inf")
    weight = torch.minimum(weight, threshold).unsqueeze(-1) * c["simi_pow"]
    weight = torch.nn.functional.softmax(weight, dim=1)
    user_emb = torch.sum(torch.multiply(weight, interests), dim=1)
    pos = torch.sum(user_emb * item_emb[:B], dim=-1, keepdim=True)  # match_model.py:54-64
    neg = torch.matmul(user_emb, item_emb[B:].T)
    sim = torch.cat([pos, neg], dim=-1) / c["temperature"]
    loss = nn.CrossEntropyLoss()(sim, torch.zeros(B, dtype=torch.long))
    loss.backward()
    return {"high": [high.detach()], "mask": mask, "sim": [sim.detach()], "loss": [loss.detach()], "gx": [xu.grad, hist.grad, xv.grad],
            "gparam": [p.grad.clone() for _, p in mod.named_parameters()]}


def main():
    from make_reference_module_vectors import _np, install_reference_imports

    install_reference_imports()
    MLP = importlib.import_module("tzrec.modules.mlp").MLP
    CapsuleLayer = importlib.import_module("tzrec.modules.capsule").CapsuleLayer
    torch.manual_seed(20261021)
    torch.set_num_threads(1)
    out = {}
    for tag, c in CASES.items():
        mod = nn.ModuleDict({"user_tower": UserTower(MLP, CapsuleLayer, c), "item_tower": ItemTower(MLP, c)})
        B, M, Lmax = len(LENGTHS), len(LENGTHS) + c["N"], max(LENGTHS)
        lengths = torch.tensor(LENGTHS, dtype=torch.int64)
        xu, xv = torch.randn(B, c["Du"]), torch.randn(M, c["Dv"])
        hist = torch.randn(B, Lmax, c["Dh"]) * (torch.arange(Lmax)[None, :] < lengths[:, None]).unsqueeze(-1).float()  # zero padded
        r32 = run(mod, c, xu, hist, lengths, xv)
        # float64: the same modules; the float64 draw under the same seed is another stream, so the fp32 draw is handed over
        torch.manual_seed(DRAW_SEED)
        drawn = torch.randn(B, c["max_seq_len"], c["max_k"])
        mod64 = copy.deepcopy(mod).double()
        if c["routing_init_method"] == "normal":
            cap_mod = sys.modules["tzrec.modules.capsule"]
            orig = cap_mod._init_routing_logits
            cap_mod._init_routing_logits = lambda x, k, init_method="normal": drawn.to(x.dtype)
            try:
                again = run(mod, c, xu, hist, lengths, xv)  # (the recorded draw IS the layer's: the fp32 run repeats bit for bit)
                assert torch.equal(again["sim"][0], r32["sim"][0]) and torch.equal(again["high"][0], r32["high"][0])
                r64 = run(mod64, c, xu.double(), hist.double(), lengths, xv.double())
            finally:
                cap_mod._init_routing_logits = orig
            out[f"{tag}/logits0"] = _np(drawn)
        else:
            r64 = run(mod64, c, xu.double(), hist.double(), lengths, xv.double())
        out[f"{tag}/xu"], out[f"{tag}/hist"], out[f"{tag}/lengths"], out[f"{tag}/xv"] = _np(xu), _np(hist), _np(lengths), _np(xv)
        out[f"{tag}/high"], out[f"{tag}/mask"] = _np(r32["high"][0]), _np(r32["mask"])
        out[f"{tag}/sim"], out[f"{tag}/loss"] = _np(r32["sim"][0]), _np(r32["loss"][0])
        out[f"{tag}/gxu"], out[f"{tag}/ghist"], out[f"{tag}/gxv"] = (_np(g) for g in r32["gx"])
        for (n, p), g in zip(mod.named_parameters(), r32["gparam"]):
            out[f"{tag}/param/{n}"], out[f"{tag}/gparam/{n}"] = _np(p), _np(g)
        for kind in KINDS:
            gap = max(float(((a.double() - e).abs() / e.abs().clamp(min=1.0)).max()) for a, e in zip(r32[kind], r64[kind]))
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_mind_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
