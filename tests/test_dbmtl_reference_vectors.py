"""ConfigDBMTL's towers against what the reference's own modules computed (tests/golden/reference_dbmtl_vectors.npz, written by
tests/golden/make_reference_dbmtl_vectors.py: tzrec.modules.mlp.MLP and nn.Linear wired as DBMTL.predict wires them): the
parameters are loaded BY NAME -- the reference's keys, its MLP's `mlp.<i>.perceptron.0` being this package's `mlp.<2i>` --, and
logits and every gradient meet the reference's within 4 x its own distance to float64 (`ref_gap`), floor 2^-20, relative to
max(1, |value|); on the fused relation chain and on the literal form."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch import nn

from cross_v2_ref import FLOOR, rel_err
from torcheasyrec_amd import _lib, rank_model
from torcheasyrec_amd.config import parse_text_proto
from torcheasyrec_amd.rank_model import ConfigDBMTL

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_reference_dbmtl_vectors import CASES  # noqa: E402  (the towers of every case; importing it runs nothing of the reference)

VEC = np.load(os.path.join(GOLDEN, "reference_dbmtl_vectors.npz"))


def _ours(ref_key):
    return re.sub(r"mlp\.(\d+)\.perceptron\.0\.", lambda m: f"mlp.{2 * int(m.group(1))}.", ref_key)


class Towers(ConfigDBMTL):
    """the towers of a ConfigDBMTL and nothing below them: every tower reads the one input"""

    def __init__(self, towers, d_in):
        nn.Module.__init__(self)
        self._losses = []
        text = ""
        for name, hidden, rel, rel_hidden in towers:
            text += f'task_towers {{ tower_name: "{name}" label_name: "{name}"'
            text += f" mlp {{ hidden_units: {hidden} }}" if hidden is not None else ""
            text += "".join(f' relation_tower_names: "{r}"' for r in rel)
            text += f" relation_mlp {{ hidden_units: {rel_hidden} }}" if rel_hidden is not None else ""
            text += " }\n"
        self._build_bayes_towers(parse_text_proto(text), d_in)

    def forward(self, x):
        task_net = [self.task_mlps[name](x) if name in self.task_mlps else x for name, _ in self._towers]
        return [self.task_outputs[i](r) for i, r in enumerate(self._relation_outputs(task_net))]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_towers_meet_the_references_vectors(dev, monkeypatch, tag, fused):
    monkeypatch.setattr(rank_model, "FUSED_RELATION_CHAIN", fused)
    B, d_in, towers = CASES[tag]
    model = Towers(towers, d_in).to(dev)
    params = {k[len(tag) + 7:]: VEC[k] for k in VEC.files if k.startswith(f"{tag}/param/")}
    state = model.state_dict()
    assert sorted(_ours(k) for k in params) == sorted(state)  # the reference's names, all of them and no other
    model.load_state_dict({_ours(k): torch.from_numpy(v) for k, v in params.items()})
    L = _lib.lib()
    orig, n_calls = L.tzr_relation_chain_fwd, [0]

    def counted(*a):
        n_calls[0] += 1
        return orig(*a)

    L.tzr_relation_chain_fwd = counted
    try:
        x = torch.from_numpy(VEC[f"{tag}/x"]).to(dev).requires_grad_(True)
        ys = model(x)
        torch.autograd.backward(ys, [torch.from_numpy(VEC[f"{tag}/gy{i}"]).to(dev) for i in range(len(towers))])
    finally:
        L.tzr_relation_chain_fwd = orig
    assert n_calls[0] == (1 if fused else 0)
    named = dict(model.named_parameters())
    got = {"y": [y.detach() for y in ys], "gx": [x.grad], "gparam": [named[_ours(k)].grad for k in sorted(params)]}
    want = {"y": [torch.from_numpy(VEC[f"{tag}/y{i}"]).double() for i in range(len(towers))], "gx": [torch.from_numpy(VEC[f"{tag}/gx"]).double()],
            "gparam": [torch.from_numpy(VEC[f"{tag}/gparam/{k}"]).double() for k in sorted(params)]}
    bad = []
    for kind in ("y", "gx", "gparam"):
        err, bound = rel_err(got[kind], want[kind]), max(4.0 * float(VEC[f"ref_gap/{tag}/{kind}"]), FLOOR)
        print(f"{tag} fused={fused} on {dev.type} {kind}: err {err:.3e} ref_gap {float(VEC[f'ref_gap/{tag}/{kind}']):.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, bad
