"""ConfigDSSM's towers and similarity head against what the reference's own modules computed
(tests/golden/reference_dssm_vectors.npz, written by tests/golden/make_reference_dssm_vectors.py: tzrec.modules.mlp.MLP and
nn.Linear wired as the reference's DSSM wires them, through normalize, sim, temperature and CrossEntropyLoss): the parameters
are loaded BY NAME -- the reference's keys, its MLP's `mlp.<i>.perceptron.0` being this package's `mlp.<2i>` --, and scores,
loss and every gradient meet the reference's within 4 x its own distance to float64 (`ref_gap`), floor 2^-20, relative to
max(1, |value|); on the fused head and on the literal form."""
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
from torcheasyrec_amd.match import ConfigDSSM, DSSMTower

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_reference_dssm_vectors import CASES  # noqa: E402  (importing it runs nothing of the reference)

VEC = np.load(os.path.join(GOLDEN, "reference_dssm_vectors.npz"))


def _ours(ref_key):
    return re.sub(r"mlp\.(\d+)\.perceptron\.0\.", lambda m: f"mlp.{2 * int(m.group(1))}.", ref_key)


class BareTower(DSSMTower):
    """a DSSMTower's dense half: its embedding group's output is given"""

    def __init__(self, d_in, hidden, output_dim):
        nn.Module.__init__(self)
        self._output_dim = output_dim
        self._build_dense(d_in, parse_text_proto(f"mlp {{ hidden_units: {hidden} }}"))


class Head(ConfigDSSM):
    """the two towers' dense halves and the head of a ConfigDSSM, nothing below them"""

    def __init__(self, c):
        nn.Module.__init__(self)
        self.user_tower = BareTower(c["Du"], c["hidden"], c["output_dim"])
        self.item_tower = BareTower(c["Dv"], c["hidden"], c["output_dim"])
        self._mode = match.IN_BATCH if c["N"] is None else match.SAMPLED
        self._cosine, self._temperature, self.want_similarity = c["cosine"], c["temperature"], True


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_towers_and_head_meet_the_references_vectors(dev, monkeypatch, tag, fused):
    monkeypatch.setattr(match, "FUSED_MATCH_SOFTMAX", fused)
    c = CASES[tag]
    model = Head(c).to(dev)
    params = {k[len(tag) + 7:]: VEC[k] for k in VEC.files if k.startswith(f"{tag}/param/")}
    assert sorted(_ours(k) for k in params) == sorted(model.state_dict())  # the reference's names, all of them and no other
    model.load_state_dict({_ours(k): torch.from_numpy(v) for k, v in params.items()})
    L = _lib.lib()
    orig, n_calls = L.tzr_match_softmax_fwd, [0]

    def counted(*a):
        n_calls[0] += 1
        return orig(*a)

    L.tzr_match_softmax_fwd = counted
    try:
        xu = torch.from_numpy(VEC[f"{tag}/xu"]).to(dev).requires_grad_(True)
        xv = torch.from_numpy(VEC[f"{tag}/xv"]).to(dev).requires_grad_(True)
        w = torch.from_numpy(VEC[f"{tag}/w"]).to(dev) if f"{tag}/w" in VEC.files else None
        losses, preds = model.head(model.user_tower.embed(xu), model.item_tower.embed(xv), w)
        losses["softmax_cross_entropy"].backward()
    finally:
        L.tzr_match_softmax_fwd = orig
    assert n_calls[0] == (1 if fused else 0)
    got = {"sim": [preds["similarity"].detach()], "loss": [losses["softmax_cross_entropy"].detach()], "gx": [xu.grad, xv.grad],
           "gparam": [p.grad for _, p in sorted(model.named_parameters())]}
    want = {"sim": [VEC[f"{tag}/sim"]], "loss": [VEC[f"{tag}/loss"]], "gx": [VEC[f"{tag}/gxu"], VEC[f"{tag}/gxv"]],
            "gparam": [VEC[f"{tag}/gparam/{k}"] for k in sorted(params, key=_ours)]}
    bad = []
    for kind in ("sim", "loss", "gx", "gparam"):
        err = rel_err([g.cpu() for g in got[kind]], [torch.from_numpy(np.asarray(e)).double() for e in want[kind]])
        bound = max(4.0 * float(VEC[f"ref_gap/{tag}/{kind}"]), FLOOR)
        print(f"{tag} fused={fused} {kind}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, bad
