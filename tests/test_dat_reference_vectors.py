"""ConfigDAT's towers, similarity head and Adaptive-Mimic loss against what the reference's own modules computed
(tests/golden/reference_dat_vectors.npz, written by tests/golden/make_reference_dat_vectors.py: tzrec.modules.mlp.MLP and nn.Linear
wired as the reference's DAT wires them, through the cat, normalize, sim, temperature, CrossEntropyLoss and the two AMM terms): the
parameters are loaded BY NAME -- the reference's keys, its MLP's `mlp.<i>.perceptron.0` being this package's `mlp.<2i>` --, and
scores, the three losses and every gradient of their sum meet the reference's within 4 x its own distance to float64 (`ref_gap`),
floor 2^-20, relative to max(1, |value|); on the fused AMM kernel and on the literal form."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch import nn

from mlp_ref import FLOOR, rel_err  # (NaN-aware: a non-finite result is an error of NaN, which fails)
from torcheasyrec_amd import _lib, match
from torcheasyrec_amd.config import parse_text_proto
from torcheasyrec_amd.match import ConfigDAT, DATTower

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_reference_dat_vectors import CASES  # noqa: E402  (importing it runs nothing of the reference)

VEC = np.load(os.path.join(GOLDEN, "reference_dat_vectors.npz"))


def _ours(ref_key):
    return re.sub(r"mlp\.(\d+)\.perceptron\.0\.", lambda m: f"mlp.{2 * int(m.group(1))}.", ref_key)


class BareTower(DATTower):
    """a DATTower's dense half: its embedding group's outputs are given, the "batch" is the dict that holds them"""

    def __init__(self, d_in, d_aug, hidden, output_dim, group, augment):
        nn.Module.__init__(self)
        self._output_dim, self._group_name, self._augment_group_name = output_dim, group, augment
        self._build_dense(d_in + d_aug, parse_text_proto(f"mlp {{ hidden_units: {hidden} }}"))

    def build_input(self, batch):
        return batch


class Model(ConfigDAT):
    """the two towers' dense halves, the head and the AMM loss of a ConfigDAT, nothing below them"""

    def __init__(self, c):
        nn.Module.__init__(self)
        D = c["output_dim"]
        self.user_tower = BareTower(c["Du"], D, c["hidden"], D, "xu", "au")
        self.item_tower = BareTower(c["Dv"], D, c["hidden"], D, "xv", "av")
        self._mode = match.IN_BATCH if c["N"] is None else match.SAMPLED
        self._cosine, self._temperature, self.want_similarity = c["cosine"], c["temperature"], True
        self._amm_u, self._amm_i = c["amm_u"], c["amm_i"]

    def _weights(self, batch):
        return batch.get("w")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_towers_head_and_amm_meet_the_references_vectors(dev, monkeypatch, tag, fused):
    monkeypatch.setattr(match, "FUSED_AMM_LOSS", fused)
    c = CASES[tag]
    assert c["B"] <= 9 and max(c["Du"], c["Dv"], *c["hidden"], c["output_dim"]) <= 25
    model = Model(c).to(dev)
    params = {k[len(tag) + 7:]: VEC[k] for k in VEC.files if k.startswith(f"{tag}/param/")}
    assert sorted(_ours(k) for k in params) == sorted(model.state_dict())  # the reference's names, all of them and no other
    model.load_state_dict({_ours(k): torch.from_numpy(v) for k, v in params.items()})
    batch = {k: torch.from_numpy(VEC[f"{tag}/{k}"]).to(dev).requires_grad_(True) for k in ("xu", "au", "xv", "av")}
    if f"{tag}/w" in VEC.files:
        batch["w"] = torch.from_numpy(VEC[f"{tag}/w"]).to(dev)
    assert ("w" in batch) == c["weights"]
    L = _lib.lib()
    orig, n_calls = L.tzr_amm_loss_fwd, [0]

    def counted(*a):
        n_calls[0] += 1
        return orig(*a)

    L.tzr_amm_loss_fwd = counted
    try:
        losses, preds = model.loss_and_predictions(batch)
        sum(losses.values()).backward()
    finally:
        L.tzr_amm_loss_fwd = orig
    assert n_calls[0] == (1 if fused else 0) and sorted(losses) == ["amm_loss_i", "amm_loss_u", "softmax_cross_entropy"]
    names = ("xu", "au", "xv", "av")
    got = {"sim": [preds["similarity"].detach()], "loss": [losses[k].detach() for k in ("softmax_cross_entropy", "amm_loss_u", "amm_loss_i")],
           "gx": [batch[k].grad for k in names], "gparam": [p.grad for _, p in sorted(model.named_parameters())]}
    want = {"sim": [VEC[f"{tag}/sim"]], "loss": [VEC[f"{tag}/{k}"] for k in ("loss", "amm_u", "amm_i")], "gx": [VEC[f"{tag}/g{k}"] for k in names],
            "gparam": [VEC[f"{tag}/gparam/{k}"] for k in sorted(params, key=_ours)]}
    bad = []
    for kind in ("sim", "loss", "gx", "gparam"):
        err = rel_err([g.cpu() for g in got[kind]], [torch.from_numpy(np.asarray(e)).double() for e in want[kind]])
        bound = max(4.0 * float(VEC[f"ref_gap/{tag}/{kind}"]), FLOOR)
        print(f"{tag} fused={fused} {kind}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, bad
