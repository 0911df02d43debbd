"""ConfigRocketLaunching's dense half -- share MLP, booster and light nets, the two logits layers, the classification losses of both
sides and the distillation terms -- against what the reference's own modules computed (tests/golden/reference_rocket_vectors.npz,
written by tests/golden/make_reference_rocket_vectors.py: tzrec.modules.mlp.MLP with return_hidden_layer_feature and nn.Linear
wired as the reference's RocketLaunching wires them): the parameters are loaded BY NAME -- the reference's keys, its MLP's
`mlp.<i>.perceptron.0` being this package's `mlp.<2i>` --, and every prediction, every loss and every gradient of the losses' sum
meet the reference's within 4 x its own distance to float64 (`ref_gap`), floor 2^-20, relative to max(1, |value|); on the fused
distillation kernel and on the literal form."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch import nn

from mlp_ref import FLOOR, rel_err  # (NaN-aware: a non-finite result is an error of NaN, which fails)
from torcheasyrec_amd import _lib, rocket
from torcheasyrec_amd.config import LossSpec
from torcheasyrec_amd.dlrm import MLP
from torcheasyrec_amd.losses import Loss
from torcheasyrec_amd.rocket import ConfigRocketLaunching

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_reference_rocket_vectors import CASES, pairs  # noqa: E402  (importing it runs nothing of the reference)

VEC = np.load(os.path.join(GOLDEN, "reference_rocket_vectors.npz"))


def _ours(ref_key):
    return re.sub(r"mlp\.(\d+)\.perceptron\.0\.", lambda m: f"mlp.{2 * int(m.group(1))}.", ref_key)


class Spec:
    def __init__(self, num_class):
        self.num_class = num_class


class Model(ConfigRocketLaunching):
    """a ConfigRocketLaunching above its embedding group: the group's rows are given, the "batch" is the object that holds them"""

    def __init__(self, c):
        nn.Module.__init__(self)
        kind = "binary_cross_entropy" if c["num_class"] == 1 else "softmax_cross_entropy"
        ls = LossSpec(kind, {"label_smoothing": 0.0})
        self._spec, self._group = Spec(c["num_class"]), "x"
        self._weight = "w" if c["weights"] else None
        self._model_losses = [Loss(ls, "y", self._weight, None)]
        self._feature_based, self._cosine = True, c["cosine"]
        d = c["D"]
        self.share_mlp = MLP(d, c["share"]) if c["share"] else None
        d = c["share"][-1] if c["share"] else d
        self.booster_mlp = MLP(d, c["booster"], return_hidden_layer_feature=True)
        self.booster_linear = nn.Linear(c["booster"][-1], c["num_class"])
        self.light_mlp = MLP(d, c["light"], return_hidden_layer_feature=True)
        self.light_linear = nn.Linear(c["light"][-1], c["num_class"])
        self.mlp_index_dict = pairs(c)
        self._pairs = sorted(self.mlp_index_dict.items())
        self._side_losses = {}
        for suffix in ("_booster", "_light"):
            sl = Loss(ls, "y", self._weight, None)
            sl.suffix, sl.name = suffix, kind + suffix
            self._side_losses[suffix] = [sl]

    def build_input(self, batch):
        return {"x": batch.x}


class Rows:
    def __init__(self, x, y, w):
        self.x, self.labels, self.sample_weights = x, {"y": y}, ({"w": w} if w is not None else {})


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_nets_losses_and_distillation_meet_the_references_vectors(dev, monkeypatch, tag, fused):
    monkeypatch.setattr(rocket, "FUSED_DISTILL_LOSS", fused)
    c = CASES[tag]
    assert c["B"] <= 9 and max(c["D"], *c["booster"], *c["light"]) <= 32
    model = Model(c).to(dev)
    params = {k[len(tag) + 7:]: VEC[k] for k in VEC.files if k.startswith(f"{tag}/param/")}
    assert sorted(_ours(k) for k in params) == sorted(model.state_dict())  # the reference's names, all of them and no other
    model.load_state_dict({_ours(k): torch.from_numpy(v) for k, v in params.items()})
    x = torch.from_numpy(VEC[f"{tag}/x"]).to(dev).requires_grad_(True)
    w = torch.from_numpy(VEC[f"{tag}/w"]).to(dev) if f"{tag}/w" in VEC.files else None
    assert (w is not None) == c["weights"]
    batch = Rows(x, torch.from_numpy(VEC[f"{tag}/y"]).to(dev), w)
    L = _lib.lib()
    orig, n_calls = L.tzr_distill_loss_fwd, [0]

    def counted(*a):
        n_calls[0] += 1
        return orig(*a)

    L.tzr_distill_loss_fwd = counted
    try:
        preds = model(batch)
        losses = model.loss(preds, batch)
        sum(losses.values()).backward()
    finally:
        L.tzr_distill_loss_fwd = orig
    assert n_calls[0] == (1 if fused else 0)
    pred_keys = sorted(k[len(tag) + 6:] for k in VEC.files if k.startswith(f"{tag}/pred/"))
    loss_keys = sorted(k[len(tag) + 6:] for k in VEC.files if k.startswith(f"{tag}/loss/"))
    assert sorted(preds) == pred_keys and sorted(losses) == loss_keys  # every prediction and loss of the reference, no other
    named = dict(model.named_parameters())
    got = {"pred": [preds[k].detach() for k in pred_keys], "loss": [losses[k].detach() for k in loss_keys], "gx": [x.grad],
           "gparam": [named[_ours(k)].grad if named[_ours(k)].grad is not None else torch.zeros_like(named[_ours(k)]) for k in sorted(params)]}
    want = {"pred": [VEC[f"{tag}/pred/{k}"] for k in pred_keys], "loss": [VEC[f"{tag}/loss/{k}"] for k in loss_keys], "gx": [VEC[f"{tag}/gx"]],
            "gparam": [VEC[f"{tag}/gparam/{k}"] for k in sorted(params)]}
    bad = []
    for kind in ("pred", "loss", "gx", "gparam"):
        err = rel_err([g.cpu() for g in got[kind]], [torch.from_numpy(np.asarray(e)).double() for e in want[kind]])
        bound = max(4.0 * float(VEC[f"ref_gap/{tag}/{kind}"]), FLOOR)
        print(f"{tag} fused={fused} {kind}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, bad
