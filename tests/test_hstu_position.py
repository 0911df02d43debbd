"""hstu.add_timestamp_positional_embeddings / add_positional_embeddings (tzr_hstu_pos_fwd / _bwd, csrc/hstu_position.hip) against
the row-by-row rule in float64 on the CPU (tests/hstu_position_ref.py): out, dx and the two table gradients under a random
upstream gradient.  Per kind: max |got - fp64| / max(1, |fp64|) at or below 4 x the distance of the same rule run in float32
(bf16 cases: run in bf16 on the bf16-rounded values, the rule of tests/test_hstu_attention_bf16.py), floor 2^-20.  The timestamps
sit away from the buckets' edges, so a row in a neighbouring bucket is an O(1) miss.  The lengths sit on the edges of the kernels'
HSTU_POS_SLAB-row slabs."""
import pytest
import torch

import hstu_position_ref as ref
from torcheasyrec_amd import _lib

BF = torch.bfloat16
SLAB = _lib.HSTU_POS_SLAB
EDGES = [0, 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1]
SHORT = [0, 1, 5, 3]  # (the widest rows: the emulator's sake)
MIXED = [0, 1, 5, SLAB, 3, 20]  # targets per sample of EDGES: two equal to n
HALF = [0, 1, 10, 20, 30, 60]  # under interleave_targets: 2 t up to n, once above it (high < 0)
BASE = dict(lengths=EDGES, E=8, P=200, T=12, max_seq_len=200, num_targets=None, interleave=False, c=0, fn="sqrt", given_query=False,
            equal=False, sliced=False, dtype=torch.float32)
CASES = {
    "base": dict(), "E4": dict(E=4), "E36": dict(E=36), "E512": dict(E=_lib.HSTU_POS_MAX_DIM, lengths=SHORT),
    "targets_zero": dict(num_targets=[0] * 6), "targets_mixed": dict(num_targets=MIXED), "interleave": dict(num_targets=HALF, interleave=True),
    "contextual_3": dict(c=3, num_targets=MIXED), "contextual_70": dict(c=70, num_targets=MIXED), "P_small": dict(P=5, c=3, num_targets=MIXED),
    "P1": dict(P=1), "T1": dict(T=1), "log": dict(fn="log", num_targets=MIXED), "query_time_given": dict(given_query=True),
    "all_timestamps_equal": dict(equal=True), "longer_than_max_seq_len": dict(max_seq_len=SLAB + 6, num_targets=MIXED, c=3),
    "column_slice": dict(sliced=True, num_targets=MIXED), "empty_batch": dict(lengths=[]),
    "pos_base": dict(T=None), "pos_targets_mixed": dict(T=None, num_targets=MIXED), "pos_interleave": dict(T=None, num_targets=HALF, interleave=True),
    "pos_P_small": dict(T=None, P=5), "pos_P1": dict(T=None, P=1), "pos_longer_than_max_seq_len": dict(T=None, max_seq_len=SLAB + 6),
    "bf16_base": dict(dtype=BF, num_targets=MIXED, c=3), "bf16_slab_edge": dict(dtype=BF, lengths=[SLAB, SLAB + 1], P=40),
    "bf16_pos": dict(dtype=BF, T=None, num_targets=MIXED[:2], lengths=[SLAB + 1, 3]),
}
_DRAWN = {}


def draw(name, **over):
    """the case's inputs, the float64 truth and the yardstick's gaps, computed once a case"""
    key = (name, repr(sorted(over.items())))
    if key not in _DRAWN:
        c = {**BASE, **CASES.get(name, {}), **over}
        p = ref.draw(c["lengths"], c["E"], c["P"], c["T"], c["max_seq_len"], sorted(CASES).index(name) if name in CASES else 99, c["num_targets"],
                     c["interleave"], c["c"], c["fn"], given_query=c["given_query"], equal=c["equal"])
        if c["dtype"] == BF:  # the truth is computed from the values the kernel sees
            for k in ("x", "g", "pos", "ts"):
                p[k] = None if p[k] is None else p[k].to(BF).float()
        want = ref.literal(p)
        lit = ref.literal(p, c["dtype"])
        kinds = tuple(k for k in ("out", "dx", "dpos", "dts") if k in want)
        _DRAWN[key] = c, p, want, {k: ref.rel_err([t.double() for t in lit[k]], want[k]) for k in kinds}, kinds
    return _DRAWN[key]


def run(dev, c, p, fused=True):
    from torcheasyrec_amd import hstu

    dt = c["dtype"]
    x, pos = (p[k].to(dev, dt).requires_grad_(True) for k in ("x", "pos"))
    ts = None if p["ts"] is None else p["ts"].to(dev, dt).requires_grad_(True)
    xin = torch.cat([torch.zeros_like(x), x, torch.zeros_like(x)], dim=1)[:, x.shape[1]:2 * x.shape[1]] if c["sliced"] else x
    opt = lambda t: None if t is None else t.to(dev)  # noqa: E731
    off, lengths = p["offsets"].to(dev), (p["offsets"][1:] - p["offsets"][:-1]).to(dev)
    before = hstu._HstuPositionFn.calls
    if ts is None:
        out = hstu.add_positional_embeddings(p["alpha"], p["max_seq_len"], pos, off, lengths, xin, opt(p["num_targets"]), p["interleave"])
    else:
        out = hstu.add_timestamp_positional_embeddings(p["alpha"], p["max_seq_len"], p["c"], pos, ts, off, lengths, xin, p["timestamps"].to(dev),
                                                       opt(p["num_targets"]), p["interleave"], p["fn"], p["incr"], opt(p["query_time"]))
    assert hstu._HstuPositionFn.calls == before + (1 if fused else 0)  # (the kernels, or the literal form)
    leaves = [x, pos] + ([] if ts is None else [ts])
    grads = torch.autograd.grad((out.float() * p["g"].to(dev)).sum(), leaves)
    assert all(t.dtype == dt for t in (out, *grads))
    return {k: [t.detach().cpu().double()] for k, t in zip(("out", "dx", "dpos", "dts"), (out, *grads))}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64(dev, name):
    c, p, want, gaps, kinds = draw(name)
    got = run(dev, c, p)
    ref.check(got, want, gaps, f"{name} on {dev.type}", kinds)
    offsets = p["offsets"].tolist()
    for b, n in enumerate(c["lengths"]):  # rows behind max_seq_len: alpha x alone, dx = alpha g
        behind = slice(offsets[b] + min(n, c["max_seq_len"]), offsets[b + 1])
        assert torch.equal(got["out"][0][behind], (p["x"][behind].to(c["dtype"]) * p["alpha"]).double())


def test_two_runs_are_bit_equal(dev):
    c, p, _, _, kinds = draw("contextual_3", equal=True)
    a, b = run(dev, c, p), run(dev, c, p)
    assert all(torch.equal(a[k][0], b[k][0]) for k in kinds)


def test_outside_the_limits_and_with_the_switch_off_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import hstu

    assert hstu.hstu_position_limit(512, 8192, 4096, 2048, 6) is None and "embedding_dim" in hstu.hstu_position_limit(12, 8, 16, dtype=BF)
    assert "dtype" in hstu.hstu_position_limit(8, 8, 16, dtype=torch.float16) and "time buckets" in hstu.hstu_position_limit(8, 8, 16, 0)
    c, p, want, gaps, kinds = draw("E6", E=6, lengths=SHORT, num_targets=[0, 1, 2, 0])  # E = 6: no multiple of 4
    ref.check(run(dev, c, p, fused=False), want, gaps, "literal E 6", kinds)
    monkeypatch.setattr(hstu, "FUSED_HSTU_POSITION", False)
    for name in ("contextual_3", "pos_targets_mixed"):
        c, p, want, gaps, kinds = draw(name)
        ref.check(run(dev, c, p, fused=False), want, gaps, f"switch off, {name}", kinds)


@pytest.mark.parametrize("use_time", [False, True])
def test_the_encoder_module_has_the_reference_names_and_equals_the_op(dev, use_time):
    from torcheasyrec_amd import hstu

    c, p, _, _, _ = draw("contextual_3")
    enc = hstu.HSTUPositionalEncoder(8, 200, 12, use_time_encoding=use_time, contextual_seq_len=3).to(dev)
    assert list(enc.state_dict()) == ["_position_embeddings_weight"] + (["_timestamp_embeddings_weight"] if use_time else [])
    assert enc._position_embeddings_weight.shape == (200, 8) and float(enc._position_embeddings_weight.detach().abs().max()) <= 200 ** -0.5
    off, x, tm, nt = (p[k].to(dev) for k in ("offsets", "x", "timestamps", "num_targets"))
    got = enc(p["max_seq_len"], off[1:] - off[:-1], off, tm, x, nt)
    if use_time:
        want = hstu.add_timestamp_positional_embeddings(8 ** 0.5, p["max_seq_len"], 3, enc._position_embeddings_weight, enc._timestamp_embeddings_weight,
                                                        off, None, x, tm, nt, False)
    else:
        want = hstu.add_positional_embeddings(8 ** 0.5, p["max_seq_len"], enc._position_embeddings_weight, off, None, x, nt, False)
    assert torch.equal(got, want) and got.requires_grad
