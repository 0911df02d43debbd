"""sequence.MultiWindowDINEncoder on the jagged rows (tzr_mwdin_fwd / _bwd, csrc/mwdin.hip) against the reference's padded form in
float64 on the CPU (tests/mwdin_ref.py): the output and every gradient (rows, query, every layer, w3 / b3, slopes, alpha) under a
random upstream gradient.  Per kind: max |got - fp64| / max(1, |fp64|) at or below 4 x the literal fp32 form's own distance to
float64 on the same inputs, floor 2^-20.  Every batch holds a sample longer than the padded length T: the divisor takes its
untruncated length, as the padded form's `sequence_length` does (embedding_group hands the lookup's lengths over as they are)."""
import pytest
import torch

import mwdin_ref as ref
from torcheasyrec_amd import _lib

W5 = [1, 1, 2, 4, 9]  # Sw = 17 crosses a 16-row block
W10 = [1, 1, 1, 2, 2, 2, 5, 6, 10, 20]
EDGES = [0, 1, 2, 4, 8, 3, 5, 9, 17, 20, 22]  # 0, 1, each cum_w, each cum_w + 1, Sw, Sw + 3, T + 2 at W5, T = 20
BASE = dict(lengths=EDGES, windows=W5, T=20, C=8, hidden=[8, 4], prelu=True, Dq=None, strided=False)
CASES = {
    "relu": dict(prelu=False), "prelu": dict(),
    "one_window": dict(windows=[1]), "window_16": dict(windows=[16]), "window_17": dict(windows=[17]),
    "ten_windows_T_below_Sw": dict(windows=W10, T=12, lengths=[0, 1, 11, 12, 13, 14, 30]),
    "ten_windows_T_above_Sw": dict(windows=W10, T=60, lengths=[0, 7, 29, 30, 31, 49, 50, 51, 60, 62]),
    "C4": dict(C=4), "C20": dict(C=20), "C128": dict(C=128),
    "h4": dict(hidden=[4]), "h36": dict(hidden=[36]), "h128": dict(hidden=[128]), "h16_8_4": dict(hidden=[16, 8, 4]), "h36_relu": dict(hidden=[36], prelu=False),
    "query_narrower": dict(Dq=4), "column_slice": dict(strided=True),
    "one_more_than_the_backward_grid": dict(lengths=[(3 * i) % 5 for i in range(_lib.MWDIN_BWD_MAX_GRID + 1)], windows=[1, 2], T=4, C=4, hidden=[4]),
}


def encoder(p, dev):
    from torcheasyrec_amd.sequence import MultiWindowDINEncoder

    hidden, C = [w.shape[0] for w in p["W"]], p["x"].shape[1]
    enc = MultiWindowDINEncoder(C, p["q"].shape[1], "g", p["windows"], {"hidden_units": hidden, "activation": "nn.ReLU" if p["slope"][0] is None else "nn.PReLU"})
    state = {"linear.weight": p["w3"], "linear.bias": p["b3"], "active.weight": p["alpha"]}
    for l in range(len(hidden)):
        state[f"mlp.mlp.{2 * l}.weight"], state[f"mlp.mlp.{2 * l}.bias"] = p["W"][l], p["b"][l]
        if p["slope"][l] is not None:
            state[f"mlp.mlp.{2 * l + 1}.weight"] = p["slope"][l]
    assert set(state) | {"windows_len", "cumsum_windows_len"} == set(enc.state_dict())  # the reference's names
    enc.load_state_dict(state, strict=False)
    return enc.to(dev)


def run(dev, p, strided=False, fused=True):
    from torcheasyrec_amd.sequence import _MwdinFn

    enc, x, C = encoder(p, dev), p["x"], p["x"].shape[1]
    if strided:  # the column slice [:, 4 : 4 + C] of a buffer 12 wider
        buf = torch.zeros(x.shape[0], C + 12)
        buf[:, 4:4 + C] = x
        x = buf.to(dev)[:, 4:4 + C]
    x, q = x.to(dev).requires_grad_(True), p["q"].to(dev).requires_grad_(True)
    before = _MwdinFn.calls
    out = enc({"g.query": q, "g.sequence_jagged": x, "g.sequence_offsets": p["offsets"].to(dev), "g.sequence_max_len": p["T"]})
    assert _MwdinFn.calls == before + (1 if fused else 0)  # (the kernel, or the literal form)
    lin = enc.mlp.linears()
    slopes = [m.weight for m in enc.mlp.mlp if isinstance(m, torch.nn.PReLU)]
    leaves = [x, q, *[m.weight for m in lin], *[m.bias for m in lin], enc.linear.weight, enc.linear.bias, *slopes, enc.active.weight]
    gr, nl = torch.autograd.grad((out * p["g"].to(dev)).sum(), leaves), len(lin)
    return {"out": [out.detach()], "dK": [gr[0]], "dQ": [gr[1]], "dW": gr[2:2 + nl], "db": gr[2 + nl:2 + 2 * nl], "dw3": [gr[2 + 2 * nl]],
            "db3": [gr[3 + 2 * nl]], "dslope": gr[4 + 2 * nl:-1], "dalpha": [gr[-1]]}


def kinds(p):
    return tuple(k for k in ref.KINDS if k != "dslope" or p["slope"][0] is not None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64(dev, name):
    c = {**BASE, **CASES[name]}
    p, want = ref.draw(c["lengths"], c["windows"], c["T"], c["C"], c["hidden"], c["prelu"], sorted(CASES).index(name), c["Dq"])
    got = run(dev, p, c["strided"])
    ref.check(got, want, ref.gaps(p, want), f"{name} on {dev.type}", kinds(p))


def test_two_runs_are_bit_equal_and_rows_behind_S_get_zero_gradients(dev):
    lengths, T = [22, 0, 40, 17, 18], 20
    p, want = ref.draw(lengths, W5, T, 8, [36], True, 50)
    a, b = run(dev, p), run(dev, p)
    for k in kinds(p):
        assert all(torch.equal(s, t) for s, t in zip(a[k], b[k])), k
    offsets = p["offsets"].tolist()
    for i, n in enumerate(lengths):
        behind = slice(offsets[i] + min(n, T, sum(W5)), offsets[i + 1])
        assert float(a["dK"][0][behind].abs().sum()) == 0.0 and float(want["dK"][0][behind].abs().sum()) == 0.0


def test_outside_the_limits_and_with_the_switch_off_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import sequence

    assert sequence.mwdin_limit(96, [36], W10, 50) is None and sequence.mwdin_limit(64, [64, 32], W10, 50) is None and sequence.mwdin_limit(8, [8, 4], W5, 20) is None
    for bad, word in ((dict(C=6), "sequence_dim"), (dict(hidden=[6]), "width"), (dict(hidden=[8] * 4), "layers"), (dict(windows=[1] * 33), "windows"),
                      (dict(windows=[200], T=200), "max_len"), (dict(C=128, windows=[128], T=128), "tile"), (dict(C=128, hidden=[128, 128, 128], T=16), "parameters")):
        c = {**dict(C=8, hidden=[8], windows=W5, T=20), **bad}
        assert word in sequence.mwdin_limit(c["C"], c["hidden"], c["windows"], c["T"]), bad
    p, want = ref.draw(EDGES, W5, 20, 8, [8, 6], True, 60)  # a width of 6: outside the limits
    ref.check(run(dev, p, fused=False), want, ref.gaps(p, want), "literal width 6", kinds(p))
    monkeypatch.setattr(sequence, "FUSED_MWDIN", False)
    p, want = ref.draw(EDGES, W5, 20, 8, [8, 4], True, 61)
    ref.check(run(dev, p, fused=False), want, ref.gaps(p, want), "switch off", kinds(p))
