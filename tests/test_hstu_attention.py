"""hstu.hstu_mha (tzr_hstu_attn_fwd / _bwd, csrc/hstu_attention.hip) against the per-sample dense form in float64 on the CPU
(tests/hstu_ref.py): the output and dq, dk, dv under a random upstream gradient.  Per kind: max |got - fp64| / max(1, |fp64|) at
or below 4 x the literal fp32 form's own distance to float64 on the same inputs, floor 2^-20.  The lengths sit on the edges of
the kernels' HSTU_BLOCK-row blocks and HSTU_TILE-key tiles."""
import pytest
import torch

import hstu_ref as ref
from torcheasyrec_amd import _lib

BLK, TILE = _lib.HSTU_BLOCK, _lib.HSTU_TILE
EDGES = [0, 1, TILE - 1, TILE, TILE + 1, BLK - 1, BLK, BLK + 1, 2 * BLK + 1]
SHORT = [0, 1, TILE + 1, 5]  # (the 128-wide cases: the emulator's sake)
MIXED = [0, 0, 3, TILE, 1, 0, 40, TILE + 1, 2 * BLK + 1]  # targets per sample of EDGES, one equal to n, one crossing a tile
BASE = dict(lengths=EDGES, H=2, Da=8, Dv=12, max_seq_len=2 * BLK + 8, num_targets=None, L=0, c=0, scaling_seqlen=-1, sliced=False)
CASES = {
    "base": dict(), "Da4": dict(Da=4), "Da20": dict(Da=20), "Da128": dict(Da=128, lengths=SHORT), "Dv4": dict(Dv=4), "Dv36": dict(Dv=36),
    "Dv128": dict(Dv=128, lengths=SHORT), "H1": dict(H=1), "H3": dict(H=3),
    "targets_0": dict(num_targets=[0] * 9), "targets_1": dict(num_targets=[0] + [1] * 8), "targets_17": dict(num_targets=[min(n, TILE + 1) for n in EDGES]),
    "targets_n": dict(num_targets=EDGES), "targets_mixed": dict(num_targets=MIXED),
    "contextual_1": dict(c=1), "contextual_3": dict(c=3), "contextual_17": dict(c=TILE + 1), "contextual_70_targets": dict(c=BLK + 6, num_targets=MIXED),
    "window_1": dict(L=1), "window_5": dict(L=5), "window_16": dict(L=TILE), "window_70": dict(L=BLK + 6),
    "all_three": dict(num_targets=MIXED, c=3, L=TILE + 4), "all_three_short_window": dict(num_targets=MIXED, c=TILE + 1, L=2),
    "scaling_seqlen": dict(scaling_seqlen=7),
    "longer_than_max_seq_len": dict(lengths=[BLK + 9, 3, TILE + 2, 2 * BLK], max_seq_len=BLK + 1, num_targets=[2, 0, 1, 70], c=2),
    "uvqk_slices": dict(sliced=True, num_targets=MIXED), "empty_batch": dict(lengths=[]),
}


def run(dev, p, sliced=False, fused=True):
    from torcheasyrec_amd import hstu

    q, k, v = (p[x].to(dev).requires_grad_(True) for x in "qkv")
    a, b, c = q, k, v
    if sliced:  # u, v, q, k as the uvqk product leaves them: column slices of one [N, (2 Dv + 2 Da) H] matrix
        (N, H, Da), Dv = q.shape, v.shape[2]
        u = torch.zeros(N, H * Dv, device=dev)
        _, c, a, b = torch.split(torch.cat([u, v.reshape(N, -1), q.reshape(N, -1), k.reshape(N, -1)], dim=1), [H * Dv, H * Dv, H * Da, H * Da], dim=1)
        a, b, c = a.view(N, H, Da), b.view(N, H, Da), c.view(N, H, Dv)
    nt = None if p["num_targets"] is None else p["num_targets"].to(dev)
    before = hstu._HstuMhaFn.calls
    out = hstu.hstu_mha(p["max_seq_len"], p["alpha"], a, b, c, p["offsets"].to(dev), num_targets=nt, max_attn_len=p["L"], contextual_seq_len=p["c"],
                        scaling_seqlen=p["scaling_seqlen"])
    assert hstu._HstuMhaFn.calls == before + (1 if fused else 0)  # (the kernels, or the literal form)
    dq, dk, dv = torch.autograd.grad((out * p["g"].to(dev)).sum(), [q, k, v])
    return {"out": [out.detach()], "dq": [dq], "dk": [dk], "dv": [dv]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64(dev, name):
    c = {**BASE, **CASES[name]}
    p, want = ref.draw(c["lengths"], c["H"], c["Da"], c["Dv"], c["max_seq_len"], sorted(CASES).index(name), c["num_targets"], c["L"], c["c"], c["scaling_seqlen"])
    got = run(dev, p, c["sliced"])
    ref.check(got, want, ref.gaps(p, want), f"{name} on {dev.type}", ref.KINDS)
    offsets = p["offsets"].tolist()
    for b, n in enumerate(c["lengths"]):  # rows behind max_seq_len: zero output, zero gradients
        behind = slice(offsets[b] + min(n, c["max_seq_len"]), offsets[b + 1])
        assert all(float(got[k][0][behind].abs().sum()) == 0.0 for k in ref.KINDS)


def test_two_runs_are_bit_equal(dev):
    p, _ = ref.draw(EDGES, 2, 8, 12, 2 * BLK + 8, 100, MIXED, TILE + 4, 3)
    a, b = run(dev, p), run(dev, p)
    assert all(torch.equal(a[k][0], b[k][0]) for k in ref.KINDS)


def test_outside_the_limits_and_with_the_switch_off_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import hstu

    assert hstu.hstu_mha_limit(4, 128, 128, 8000) is None and "attention_dim" in hstu.hstu_mha_limit(2, 6, 12, 100) and "hidden_dim" in hstu.hstu_mha_limit(2, 8, 132, 100)
    p, want = ref.draw(EDGES, 2, 6, 12, 2 * BLK + 8, 101, MIXED, TILE + 4, 3)  # Da = 6: outside the limits
    ref.check(run(dev, p, fused=False), want, ref.gaps(p, want), "literal Da 6", ref.KINDS)
    monkeypatch.setattr(hstu, "FUSED_HSTU_MHA", False)
    p, want = ref.draw(EDGES, 2, 8, 12, 2 * BLK + 8, 102, MIXED, TILE + 4, 3)
    ref.check(run(dev, p, fused=False), want, ref.gaps(p, want), "switch off", ref.KINDS)


def test_what_is_not_built_is_refused_by_name(dev):
    from torcheasyrec_amd import hstu

    p, _ = ref.draw([3], 1, 4, 4, 8, 103)
    args = (8, 0.5, p["q"].to(dev), p["k"].to(dev), p["v"].to(dev), p["offsets"].to(dev))
    for kwargs, word in ((dict(causal=False), "causal"), (dict(attn_func=torch.zeros(1, 3, 3, dtype=torch.int32)), "attn_func"),
                         (dict(dropout_pr=0.1), "dropout_pr"), (dict(min_full_attn_seq_len=2), "min_full_attn_seq_len")):
        with pytest.raises(NotImplementedError, match=word):
            hstu.hstu_mha(*args, **kwargs)
