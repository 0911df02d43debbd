"""hstu_mlps.jagged_dense_bmm_broadcast_add (tzr_jagged_bmm_fwd / _bwd, csrc/jagged_bmm.hip) and the contextualized MLPs on it
against the per-sample dense form in float64 on the CPU (tests/jagged_bmm_ref.py): out, d jagged, d dense and d bias under a random
upstream gradient.  Per kind: max |got - fp64| / max(1, |fp64|) at or below 4 x the distance of the same form run in float32,
floor 2^-20 (the rule of tests/test_hstu_attention.py).  The lengths sit on the edges of the kernels' row block and MFMA tile, the
widths on the edges of the column chunk (N forward, K in d jagged) and of the weight kernel's 64-k tile."""
import copy

import pytest
import torch
import torch.nn.functional as F

import jagged_bmm_ref as ref
from torcheasyrec_amd import _lib

R, CHUNK = _lib.JAGGED_BMM_BLOCK, _lib.JAGGED_BMM_CHUNK
EDGES = [0, 1, 15, 16, 17, R - 1, R, R + 1, 2 * R + 1]
SHORT = [0, 1, 17, 3]  # (the widest rows: the emulator's sake)
BASE = dict(lengths=EDGES, K=20, N=36, max_seq_len=200, spare=0, sliced=False, dtype=torch.float32)
CASES = {
    "base": dict(), "K4_N4": dict(K=4, N=4), "K64_N36": dict(K=64), "K4_N36": dict(K=4), "N_over_chunk": dict(N=CHUNK + 4, K=64),
    "K_over_chunk": dict(K=CHUNK + 4, lengths=SHORT + [R + 1]), "N_max": dict(N=_lib.JAGGED_BMM_MAX_DIM, K=4, lengths=SHORT),
    "K_max": dict(K=_lib.JAGGED_BMM_MAX_DIM, N=4, lengths=SHORT), "one_sample": dict(lengths=[R + 1]), "empty_batch": dict(lengths=[]),
    "all_empty": dict(lengths=[0, 0, 0]), "long_alone": dict(lengths=[R + 16], max_seq_len=R + 6), "long_mixed": dict(max_seq_len=R + 6),
    "spare_rows": dict(spare=5, max_seq_len=R + 6), "column_slices": dict(sliced=True),
}
_DRAWN = {}


def draw(name, **over):
    """the case's inputs, the float64 truth and the yardstick's gaps, computed once a case"""
    key = (name, repr(sorted(over.items())))
    if key not in _DRAWN:
        c = {**BASE, **CASES.get(name, {}), **over}
        p = ref.draw(c["lengths"], c["K"], c["N"], c["max_seq_len"], sorted(CASES).index(name) if name in CASES else 99, c["spare"])
        if c["dtype"] != torch.float32:  # the truth is computed from the values the op sees
            p.update({k: p[k].to(c["dtype"]).float() for k in ("jagged", "dense", "bias", "g")})
        want = ref.literal(p)
        _DRAWN[key] = c, p, want, ref.gaps(p, want, c["dtype"])
    return _DRAWN[key]


def run(dev, c, p, fused=True, **kw):
    from torcheasyrec_amd import hstu_mlps

    x, w, b = (p[k].to(dev, c["dtype"]).requires_grad_(True) for k in ("jagged", "dense", "bias"))
    wide = lambda t: torch.cat([torch.zeros_like(t), t, torch.zeros_like(t)], dim=1)[:, t.shape[1]:2 * t.shape[1]]  # noqa: E731
    g = p["g"].to(dev, c["dtype"])
    before = hstu_mlps._JaggedBmmFn.calls
    out = hstu_mlps.jagged_dense_bmm_broadcast_add(p["max_seq_len"], p["offsets"].to(dev), wide(x) if c["sliced"] else x, w, b, **kw)
    assert hstu_mlps._JaggedBmmFn.calls == before + (1 if fused else 0)  # (the kernels, or the literal form)
    grads = torch.autograd.grad(out, [x, w, b], grad_outputs=wide(g) if c["sliced"] else g)
    assert all(t.dtype == c["dtype"] for t in (out, *grads))
    return {k: [t.detach().cpu().double()] for k, t in zip(ref.KINDS, (out, *grads))}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64(dev, name):
    c, p, want, gaps = draw(name)
    got = run(dev, c, p)
    ref.check(got, want, gaps, f"{name} on {dev.type}", ref.KINDS)
    offsets = p["offsets"].tolist()
    dropped = [slice(offsets[b] + min(n, c["max_seq_len"]), offsets[b + 1]) for b, n in enumerate(c["lengths"])] + [slice(offsets[-1], None)]
    for rows in dropped:  # rows behind max_seq_len and spare rows: exactly zero
        assert not got["out"][0][rows].any() and not got["dj"][0][rows].any()


def test_two_runs_are_bit_equal(dev):
    c, p, _, _ = draw("base")
    a, b = run(dev, c, p), run(dev, c, p)
    assert all(torch.equal(a[k][0], b[k][0]) for k in ref.KINDS)


def test_outside_the_limits_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import hstu_mlps

    limit = hstu_mlps.jagged_bmm_limit
    assert limit(64, 512, 4096, 128) is None and limit(6, 8, 16).startswith("K 6") and limit(8, 516, 16).startswith("N 516")
    assert "max_seq_len" in limit(8, 8, 0) and "dtype" in limit(8, 8, 16, dtype=torch.bfloat16) and "grid" in limit(8, 8, 2 ** 28, 2 ** 20)
    for name, over in (("K6", dict(K=6, lengths=SHORT)), ("bf16", dict(dtype=torch.bfloat16, lengths=SHORT))):
        c, p, want, gaps = draw(name, **over)
        ref.check(run(dev, c, p, fused=False), want, gaps, f"literal {name}", ref.KINDS)
    c, p, want, gaps = draw("long_mixed")
    got = run(dev, c, p, fused=False, double_backward=True)
    monkeypatch.setattr(hstu_mlps, "FUSED_JAGGED_BMM", False)
    for got in (got, run(dev, c, p, fused=False)):
        ref.check(got, want, gaps, "literal long_mixed", ref.KINDS)
    # a second derivative through the literal form, d/d dense of <d jagged, h>: float64, the yardstick in float32, the package
    h, seconds = torch.randn(p["jagged"].shape, generator=torch.Generator().manual_seed(7)), []
    op = lambda x, w, b: hstu_mlps.jagged_dense_bmm_broadcast_add(p["max_seq_len"], p["offsets"].to(dev), x, w, b, double_backward=True)  # noqa: E731
    for to, dt, fn in (("cpu", torch.float64, lambda *a: ref.product(p, *a)), ("cpu", torch.float32, lambda *a: ref.product(p, *a)), (dev, torch.float32, op)):
        x, w, b = (p[k].to(to, dt).requires_grad_(True) for k in ("jagged", "dense", "bias"))
        dj, = torch.autograd.grad(fn(x, w, b), x, grad_outputs=p["g"].to(x), create_graph=True)
        seconds.append({"ddw": [torch.autograd.grad((dj * h.to(x)).sum(), w)[0].cpu().double()]})
    ref.check(seconds[2], seconds[0], {"ddw": ref.rel_err(seconds[1]["ddw"], seconds[0]["ddw"])}, "second derivative", ("ddw",))


PARAMETERIZED_KEYS = ("_dense_features_compress.weight", "_dense_features_compress.bias", "_attn_raw_weights.0.weight", "_attn_raw_weights.0.bias",
                      "_attn_weights_norm.weight", "_attn_weights_norm.bias", "_res_weights.0.weight", "_res_weights.0.bias",
                      "_res_weights.1.weight", "_res_weights.1.bias", "_res_weights.2.weight", "_res_weights.2.bias")


def test_the_parameterized_mlp_has_the_reference_names_and_equals_its_literal_form(dev, monkeypatch):
    from torcheasyrec_amd import hstu_mlps

    torch.manual_seed(3)
    mlp = hstu_mlps.create_contextualized_mlp({"parameterized_mlp": dict(contextual_embedding_dim=12, sequential_input_dim=8, hidden_dim=8)},
                                              sequential_output_dim=12).eval()
    assert isinstance(mlp, hstu_mlps.ParameterizedContextualizedMLP) and tuple(mlp.state_dict()) == PARAMETERIZED_KEYS
    assert not mlp._res_weights[0].bias.any() and float(mlp._res_weights[0].weight.detach().abs().max()) <= (6 / 16) ** 0.5  # xavier, zero bias
    _, p, _, _ = draw("mlp", K=8, N=12)
    ctx = torch.randn(len(EDGES), 12)

    def grads(m, to, dt, fused):
        m = copy.deepcopy(m).to(to, dt)
        before = hstu_mlps._JaggedBmmFn.calls
        out = m(p["jagged"].to(to, dt), p["offsets"].to(to), 200, ctx.to(to, dt))
        assert hstu_mlps._JaggedBmmFn.calls == before + (1 if fused else 0)
        got = (out, *torch.autograd.grad(out, list(m.parameters()), grad_outputs=p["g"].to(to, dt)))
        return {"mlp": [t.detach().cpu().double() for t in got]}

    got = grads(mlp, dev, torch.float32, True)
    monkeypatch.setattr(hstu_mlps, "FUSED_JAGGED_BMM", False)
    want = grads(mlp, "cpu", torch.float64, False)
    ref.check(got, want, {"mlp": ref.rel_err(grads(mlp, dev, torch.float32, False)["mlp"], want["mlp"])}, "parameterized mlp", ("mlp",))


def test_the_simple_mlp_is_its_four_layers(dev):
    from torcheasyrec_amd import hstu_mlps

    mlp = hstu_mlps.create_contextualized_mlp({"simple_mlp": dict(sequential_input_dim=8, sequential_output_dim=12, hidden_dim=20)}).to(dev)
    s = mlp.state_dict()
    assert tuple(s) == tuple(f"_mlp.{i}.{n}" for i in range(4) for n in ("weight", "bias"))
    x = torch.randn(9, 8).to(dev)
    h = F.linear(x, s["_mlp.0.weight"], s["_mlp.0.bias"])
    h = h * torch.sigmoid(F.layer_norm(h, [20], s["_mlp.1.weight"], s["_mlp.1.bias"], 1e-5))
    want = F.layer_norm(F.linear(h, s["_mlp.2.weight"], s["_mlp.2.bias"]), [12], s["_mlp.3.weight"], s["_mlp.3.bias"], 1e-5)
    assert torch.equal(mlp(x, torch.tensor([0, 9]).to(dev), 16, None), want)
