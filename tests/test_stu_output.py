"""hstu.stu_output (tzr_stu_output_fwd / _bwd, csrc/stu_output.hip) against the stage restated in float64 on the CPU
(tests/stu_output_ref.py): out, du, dattn, dx, dWo, dgamma, dbeta under a random upstream gradient.  Per kind: max |got - fp64| /
max(1, |fp64|) at or below 4 x the float32 restatement's own distance to float64 on the same inputs, floor 2^-20.  The shapes sit
where the kernels' row blocks, 16-column tiles and width classes end."""
import functools

import pytest
import torch

import stu_output_ref as ref
from torcheasyrec_amd import _lib

BLK = _lib.STU_OUT_BLOCK
CASES = {  # L, E, H, Dv, group norm, p
    "one_row": (1, 12, 2, 8, False, 0.0),                     # E below one 16-column tile, W = 16
    "row_tail_smallest_group": (BLK + 1, 20, 3, 4, True, 0.0),  # W = 12: no multiple of 16
    "several_blocks": (3 * BLK + 1, 72, 2, 36, False, 0.0),   # the weight pass walks more than a step; E, W past 64 with tile tails
    "dropout": (BLK + 1, 72, 2, 36, True, 0.5),               # all three segments, forward and both backward passes, a given seed
    "both_limits": (BLK + 1, 512, 4, 128, False, 0.0),        # the accumulator and the LDS budget at once
}


@functools.lru_cache(maxsize=None)
def drawn(name, training=True):
    return ref.draw(*CASES[name], sorted(CASES).index(name), training)


def run(dev, c, monkeypatch, fused=1, seed=True, **over):
    from torcheasyrec_amd import hstu

    monkeypatch.setattr(hstu, "FUSED_STU_OUTPUT", True)
    wide = c["wide"].to(dev).requires_grad_(True)
    u = wide[:, :c["u"].shape[1]]
    attn, x, wo, gamma, beta = (c[k].to(dev).requires_grad_(True) for k in ref.LEAVES[1:])
    before = hstu._StuOutputFn.calls
    out = hstu.stu_output(u, attn, x, gamma, beta, wo, c["H"], c["group_norm"], over.get("p", c["p"]), c["training"], c["eps"],
                          seed=torch.tensor([c["seed"]], device=dev) if seed else None)
    assert hstu._StuOutputFn.calls == before + fused  # (the kernels, or the literal form)
    grads = torch.autograd.grad((out * c["g"].to(dev)).sum(), [u, attn, x, wo, gamma, beta])
    return dict(zip(ref.KINDS, [[out.detach()]] + [[t] for t in grads]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64(dev, name, monkeypatch):
    c, want, gaps = drawn(name)
    ref.check(run(dev, c, monkeypatch), want, gaps, f"{name} on {dev.type}", ref.KINDS)


def test_two_runs_are_bit_equal(dev, monkeypatch):
    c = drawn("dropout")[0]
    a, b = run(dev, c, monkeypatch), run(dev, c, monkeypatch)
    assert all(torch.equal(a[k][0], b[k][0]) for k in ref.KINDS)


def test_no_rows(dev, monkeypatch):
    c = ref.draw(0, 12, 2, 8, False, 0.3, 50)[0]
    got = run(dev, c, monkeypatch)
    assert [tuple(got[k][0].shape) for k in ref.KINDS] == [(0, 12), (0, 16), (0, 16), (0, 12), (48, 12), (16,), (16,)]
    assert all(float(got[k][0].abs().sum()) == 0.0 for k in ("dWo", "dgamma", "dbeta"))


def test_dropout_is_off_outside_training(dev, monkeypatch):
    c = drawn("dropout", False)[0]
    a, b = run(dev, c, monkeypatch), run(dev, c, monkeypatch, p=0.0)
    assert all(torch.equal(a[k][0], b[k][0]) for k in ref.KINDS)


def test_a_seed_is_drawn_when_none_is_given(dev, monkeypatch):
    c = drawn("dropout")[0]
    a, b = run(dev, c, monkeypatch, seed=False), run(dev, c, monkeypatch, seed=False)
    assert not torch.equal(a["out"][0], b["out"][0])


@pytest.mark.parametrize("shape,word", [((BLK + 1, 516, 2, 8, False, 0.0), "embedding_dim"), ((BLK + 1, 12, 2, 6, True, 0.0), "hidden_dim")])
def test_outside_the_limits_the_literal_form_runs(dev, monkeypatch, shape, word):
    from torcheasyrec_amd import hstu

    assert hstu.stu_output_limit(512, 4, 128, True) is None and word in hstu.stu_output_limit(*shape[1:5])
    c, want, gaps = ref.draw(*shape, 60)
    ref.check(run(dev, c, monkeypatch, fused=0), want, gaps, f"literal {word}", ref.KINDS)
