"""ConfigMIND's towers, label-aware attention and similarity head against what the reference's own modules computed
(tests/golden/reference_mind_vectors.npz, written by tests/golden/make_reference_mind_vectors.py: tzrec.modules.capsule.CapsuleLayer,
tzrec.modules.mlp.MLP and nn.Linear wired as the reference's MIND wires them, through label_aware_attention, the sampled
similarity and CrossEntropyLoss): the parameters are loaded BY NAME -- the reference's keys, its MLP's `mlp.<i>.perceptron.0`
being this package's `mlp.<2i>` --, the history goes in as ROWS (the reference took it padded), and the capsules, the mask, the
scores, the loss and every gradient meet the reference's within 4 x its own distance to float64 (`ref_gap`), floor 2^-20,
relative to max(1, |value|); on the fused kernels and on the literal forms.  Two cases: `zeros` init at the default routing
settings, `normal` init (the reference's drawn logits, recorded) at the reference test's."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch import nn

from mlp_ref import FLOOR, rel_err  # (NaN-aware: a non-finite result is an error of NaN, which fails)
from torcheasyrec_amd import _lib, capsule, match
from torcheasyrec_amd.config import parse_text_proto
from torcheasyrec_amd.match import ConfigMIND, MINDItemTower, MINDUserTower

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLDEN)
from make_reference_mind_vectors import CASES  # noqa: E402  (importing it runs nothing of the reference)

VEC = np.load(os.path.join(GOLDEN, "reference_mind_vectors.npz"))


def _ours(ref_key):
    return re.sub(r"mlp\.(\d+)\.perceptron\.0\.", lambda m: f"mlp.{2 * int(m.group(1))}.", ref_key)


class BareUserTower(MINDUserTower):
    """a MINDUserTower's dense half: its embedding group's outputs are given"""

    def __init__(self, c):
        nn.Module.__init__(self)
        self._output_dim, self._similarity = c["output_dim"], "COSINE"
        cap = " ".join(f"{k}: {c[k]!r}".replace("'", '"') for k in ("max_k", "max_seq_len", "high_dim", "num_iters", "routing_logits_scale",
                                                                    "routing_logits_stddev", "squash_pow", "routing_init_method"))
        self._build_dense(c["Du"], c["Dh"], parse_text_proto(
            f"user_mlp {{ hidden_units: {c['user_mlp']} }} hist_seq_mlp {{ hidden_units: {c['hist_seq_mlp']} }} "
            f"capsule_config {{ {cap} }} concat_mlp {{ hidden_units: {c['concat_mlp']} }}"))


class BareItemTower(MINDItemTower):
    def __init__(self, c):
        nn.Module.__init__(self)
        self._output_dim, self._similarity = c["output_dim"], "COSINE"
        self._build_dense(c["Dv"], parse_text_proto(f"mlp {{ hidden_units: {c['item_mlp']} }}"))


class Head(ConfigMIND):
    """the two towers' dense halves, the attention and the head of a ConfigMIND, nothing below them"""

    def __init__(self, c):
        nn.Module.__init__(self)
        self.user_tower, self.item_tower = BareUserTower(c), BareItemTower(c)
        self._mode, self._cosine, self._temperature, self._simi_pow = match.SAMPLED, True, c["temperature"], c["simi_pow"]
        self.want_similarity = True


def counted(names):
    L = _lib.lib()
    orig, calls = {n: getattr(L, n) for n in names}, {n: 0 for n in names}
    for n in names:
        setattr(L, n, (lambda n: lambda *a: (calls.__setitem__(n, calls[n] + 1), orig[n](*a))[1])(n))
    return orig, calls


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_towers_attention_and_head_meet_the_references_vectors(dev, monkeypatch, tag, fused):
    for mod, name in ((match, "FUSED_MATCH_SOFTMAX"), (match, "FUSED_LABEL_ATTENTION"), (capsule, "FUSED_CAPSULE")):
        monkeypatch.setattr(mod, name, fused)
    c = CASES[tag]
    model = Head(c).to(dev)
    params = {k[len(tag) + 7:]: VEC[k] for k in VEC.files if k.startswith(f"{tag}/param/")}
    assert sorted(_ours(k) for k in params) == sorted(model.state_dict())  # the reference's names, all of them and no other
    model.load_state_dict({_ours(k): torch.from_numpy(v) for k, v in params.items()})
    # the padded history as rows: sample b's first min(len, width) positions
    hist, lengths = torch.from_numpy(VEC[f"{tag}/hist"]), torch.from_numpy(VEC[f"{tag}/lengths"])
    keep = torch.arange(hist.shape[1])[None, :] < lengths[:, None]
    rows = hist[keep].to(dev).requires_grad_(True)
    offsets = torch.cat([lengths.new_zeros(1), lengths.cumsum(0)]).to(dev)
    logits0 = None
    if f"{tag}/logits0" in VEC.files:  # the reference's draw [B, S, K] at the positions that exist
        drawn = torch.from_numpy(VEC[f"{tag}/logits0"])
        S = drawn.shape[1]
        padded = torch.zeros(hist.shape[0], max(S, hist.shape[1]), drawn.shape[2])
        padded[:, :S] = drawn
        logits0 = padded[:, :hist.shape[1]][keep].to(dev)  # (rows behind S carry zeros: they do not exist for the layer)
    names = ("tzr_capsule_fwd", "tzr_label_attn_fwd", "tzr_match_softmax_fwd")
    orig, calls = counted(names)
    try:
        xu = torch.from_numpy(VEC[f"{tag}/xu"]).to(dev).requires_grad_(True)
        xv = torch.from_numpy(VEC[f"{tag}/xv"]).to(dev).requires_grad_(True)
        interests, mask = model.user_tower.interests(xu, rows, offsets, logits0)
        v = model.item_tower.embed(xv)
        losses, preds = model.head(match.label_attention(interests, v, mask, model._simi_pow), v)
        losses["softmax_cross_entropy"].backward()
        with torch.no_grad():
            x = rows.detach()
            x = model.user_tower._hist_seq_mlp_out(model.user_tower._hist_seq_mlp(x))
            high, mask2 = model.user_tower._capsule_layer(x, offsets, logits0)
    finally:
        for n in names:
            setattr(_lib.lib(), n, orig[n])
    assert calls == {"tzr_capsule_fwd": 2 if fused else 0, "tzr_label_attn_fwd": 1 if fused else 0, "tzr_match_softmax_fwd": 1 if fused else 0}
    assert torch.equal(mask.cpu(), torch.from_numpy(VEC[f"{tag}/mask"])) and torch.equal(mask2, mask)
    ghist = torch.zeros(hist.shape)
    ghist[keep] = rows.grad.cpu()
    got = {"high": [high], "sim": [preds["similarity"].detach()], "loss": [losses["softmax_cross_entropy"].detach()],
           "gx": [xu.grad, ghist, xv.grad], "gparam": [p.grad for _, p in sorted(model.named_parameters())]}
    want = {"high": [VEC[f"{tag}/high"]], "sim": [VEC[f"{tag}/sim"]], "loss": [VEC[f"{tag}/loss"]],
            "gx": [VEC[f"{tag}/gxu"], VEC[f"{tag}/ghist"], VEC[f"{tag}/gxv"]], "gparam": [VEC[f"{tag}/gparam/{k}"] for k in sorted(params, key=_ours)]}
    bad = []
    for kind in ("high", "sim", "loss", "gx", "gparam"):
        err = rel_err([g.cpu() for g in got[kind]], [torch.from_numpy(np.asarray(e)).double() for e in want[kind]])
        bound = max(4.0 * float(VEC[f"ref_gap/{tag}/{kind}"]), FLOOR)
        print(f"{tag} fused={fused} {kind}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, bad
