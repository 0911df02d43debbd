"""Generate tests/golden/reference_rocket_vectors.npz by RUNNING the reference's own `tzrec.modules.mlp.MLP` (with
`return_hidden_layer_feature=True`) and `nn.Linear`, wired as the reference's RocketLaunching wires them
(tzrec/models/rocket_launching.py:88-123: the optional share MLP, the light net over `share_net.detach()`, the booster over
`share_net`, the two logits layers, the paired hidden layers; rank_model.py:133-167: logits / probs per loss kind;
rocket_launching.py:125-155: `feature_based_sim`; :182-204: `_distillation_loss`; :206-245 and rank_model.py:219-262: the
classification loss of both sides, every term weighted by w / mean(w)).

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_rocket_vectors.py

`tzrec/modules/mlp.py` is imported from where it lies through the import shim of make_reference_module_vectors.py and executed
on CPU in fp32, with the modules' own initialisation; `rocket_launching.py` itself cannot be imported here (it pulls the dataset
and protobuf stack), so the wiring is this file's own words, as make_reference_dat_vectors.py wires dat.py by hand.

Per case: the feature group's rows `x` [B, D], the labels `y`, the sample weights `w` (if any), every parameter `param/<key>`
under the key the reference's RocketLaunching gives it (`share_mlp.mlp.<i>.perceptron.0.*`, `booster_mlp.*`, `light_mlp.*`,
`booster_linear.*`, `light_linear.*`), every prediction `pred/<key>`, every loss `loss/<key>`, and the gradients `gx`,
`gparam/<key>` of the losses' sum.  `ref_gap/<case>/<kind>` (kind: pred, loss, gx, gparam) is the reference's own distance to a
float64 evaluation of the same modules on the same values, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: the
yardstick the test scales its bound with.  CASES is read by the test from here.
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

# case -> dict(B, D (the group's width), share (hidden units or None), booster, light, num_class, cosine, weights)
CASES = {
    "bce_cos_share_b9": dict(B=9, D=21, share=[24], booster=[32, 16, 8], light=[16, 8], num_class=1, cosine=True, weights=False),
    "softmax_dist_b7": dict(B=7, D=21, share=None, booster=[32, 16, 8], light=[16, 8], num_class=2, cosine=False, weights=False),
    "bce_cos_share_b7_w": dict(B=7, D=21, share=[24], booster=[32, 16, 8], light=[16, 8], num_class=1, cosine=True, weights=True),
}
KINDS = ("pred", "loss", "gx", "gparam")


def pairs(c):
    """rocket_launching.py:77-86"""
    out = {}
    for i, unit_i in enumerate(c["light"]):
        for j, unit_j in enumerate(c["booster"]):
            if unit_i == unit_j:
                out[i] = j
                break
    return out


def build(MLP, c):
    """rocket_launching.py:49-73"""
    mod = nn.ModuleDict()
    d = c["D"]
    if c["share"]:
        mod["share_mlp"] = MLP(d, hidden_units=c["share"])
        d = mod["share_mlp"].output_dim()
    mod["booster_mlp"] = MLP(d, hidden_units=c["booster"], return_hidden_layer_feature=True)
    mod["booster_linear"] = nn.Linear(mod["booster_mlp"].output_dim(), c["num_class"])
    mod["light_mlp"] = MLP(d, hidden_units=c["light"], return_hidden_layer_feature=True)
    mod["light_linear"] = nn.Linear(mod["light_mlp"].output_dim(), c["num_class"])
    return mod


def to_prediction(c, out, suffix):
    """rank_model.py:133-167"""
    if c["num_class"] == 1:
        logits = torch.squeeze(out, dim=1)
        return {"logits" + suffix: logits, "probs" + suffix: torch.sigmoid(logits)}
    probs = torch.softmax(out, dim=1)
    return {"logits" + suffix: out, "probs" + suffix: probs, "probs1" + suffix: probs[:, 1]}


def div_no_nan(a, b):
    """what tzrec/modules/utils.py:94-126 computes: a / b, 0 where b is 0"""
    return torch.where(b != 0, a / torch.where(b != 0, b, torch.ones_like(b)), torch.zeros_like(a))


def run(mod, c, x, y, w):
    x = x.clone().requires_grad_(True)
    mod.zero_grad()
    # predict, training mode
    share_net = mod["share_mlp"](x) if "share_mlp" in mod else x
    light_net = mod["light_mlp"](share_net.detach())
    pred = to_prediction(c, mod["light_linear"](light_net["hidden_layer_end"]), "_light")
    booster_net = mod["booster_mlp"](share_net)
    pred.update(to_prediction(c, mod["booster_linear"](booster_net["hidden_layer_end"]), "_booster"))
    for i, j in pairs(c).items():
        pred[f"light_{i}"] = light_net["hidden_layer" + str(i)]
        pred[f"booster_{j}"] = booster_net["hidden_layer" + str(j)]
    # loss
    losses = {}
    loss_weight = None if w is None else div_no_nan(w, torch.mean(w))
    reduction = "none" if w is not None else "mean"
    for suffix in ("_booster", "_light"):
        if c["num_class"] == 1:
            name, l = "binary_cross_entropy", nn.BCEWithLogitsLoss(reduction=reduction)(pred["logits" + suffix], y.to(x.dtype))
        else:
            name, l = "softmax_cross_entropy", nn.CrossEntropyLoss(reduction=reduction)(pred["logits" + suffix], y)
        losses[name + suffix] = torch.mean(l * loss_weight) if loss_weight is not None else l
    for i, j in pairs(c).items():  # feature_based_sim
        light_feature, booster_feature_no_gradient = pred[f"light_{i}"], pred[f"booster_{j}"].detach()
        if c["cosine"]:
            multi = torch.mul(F.normalize(booster_feature_no_gradient, p=2, dim=1), F.normalize(light_feature, p=2, dim=1))
            rows = torch.sum(multi, dim=1)
            sim = -0.1 * torch.mean(rows * loss_weight if loss_weight is not None else rows)
        else:
            distance_square = torch.square(booster_feature_no_gradient - light_feature)
            if loss_weight is not None:
                distance_square = torch.sum(distance_square, dim=1) * loss_weight
            sim = torch.sqrt(torch.sum(distance_square))
        losses[f"similarity_{i}_{j}"] = sim
    hint = nn.MSELoss(reduction=reduction)(pred["logits_light"], pred["logits_booster"].detach())
    losses["hint_l2_loss"] = torch.mean(hint * loss_weight) if loss_weight is not None else hint
    sum(losses.values()).backward()
    return {"pred": {k: v.detach() for k, v in pred.items()}, "loss": {k: v.detach() for k, v in losses.items()}, "gx": {"gx": x.grad},
            "gparam": {n: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for n, p in mod.named_parameters()}}


def main():
    from make_reference_module_vectors import _np, install_reference_imports

    install_reference_imports()
    MLP = importlib.import_module("tzrec.modules.mlp").MLP
    torch.manual_seed(20261021)
    torch.set_num_threads(1)
    out = {}
    for tag, c in CASES.items():
        mod = build(MLP, c)
        x = torch.randn(c["B"], c["D"])
        y = (torch.rand(c["B"]) < 0.4).to(torch.int64)
        w = 0.5 + torch.rand(c["B"]) if c["weights"] else None
        r32 = run(mod, c, x, y, w)
        r64 = run(copy.deepcopy(mod).double(), c, x.double(), y, None if w is None else w.double())
        out[f"{tag}/x"], out[f"{tag}/y"], out[f"{tag}/gx"] = _np(x), _np(y), _np(r32["gx"]["gx"])
        if w is not None:
            out[f"{tag}/w"] = _np(w)
        for kind in ("pred", "loss"):
            for k, v in r32[kind].items():
                out[f"{tag}/{kind}/{k}"] = _np(v)
        for n, p in mod.named_parameters():
            out[f"{tag}/param/{n}"], out[f"{tag}/gparam/{n}"] = _np(p), _np(r32["gparam"][n])
        for kind in KINDS:
            gap = max(float(((r32[kind][k].double() - e).abs() / e.abs().clamp(min=1.0)).max()) for k, e in r64[kind].items())
            out[f"ref_gap/{tag}/{kind}"] = np.float64(gap)
            print(tag, kind, gap)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_rocket_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
