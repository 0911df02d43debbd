"""hstu.delta_hstu_mha (tzr_hstu_delta_fwd, csrc/hstu_delta.hip) and STULayer / STUStack.cached_forward.  The op against
hstu_ref.attention in float64 on the FULL sequences (cache + delta rows, arbitrary q in front of the delta rows), of which each
sample's last `delta` rows are compared: max |got - fp64| / max(1, |fp64|) at or below 4 x the float32 restatement's own distance,
floor 2^-20.  Every case runs in the two-segment form (cache and delta rows apart) and in the reference's one-segment form (the
full rows), and the two are bit-equal.  The cache lengths sit on the edges of the kernel's 16-key tiles, of the four waves' share
(4 tiles) and of its HSTU_DELTA_CHUNK-key chunks."""
import pytest
import torch

import hstu_ref as ref
from test_stu_layer import NAMES, layer_ref
from torcheasyrec_amd import _lib

T, C = _lib.HSTU_TILE, _lib.HSTU_DELTA_CHUNK
SHORT = [0, 1, T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1]
TINY = [0, 1, T + 1, 5]  # (the 128-wide cases: the emulator's sake)
MIXED = [0, 1, 3, 17, 18, 40, 2, 17]  # targets per sample of SHORT at delta 17: none, below, equal to and above delta
BASE = dict(cache=SHORT, delta=17, H=2, Da=8, Dv=12, max_seq_len=None, num_targets=None, L=0, c=0, scaling_seqlen=-1, sliced=False, refused=())
CASES = {
    "chunk_edges": dict(cache=[C - 1, C, C + 1, 2 * C + 1]), "delta_1": dict(delta=1), "delta_15": dict(delta=15), "delta_16": dict(delta=16),
    "delta_33": dict(delta=33, num_targets=[33] * 8), "Da4_Dv20": dict(Da=4, Dv=20), "Da20_Dv4": dict(Da=20, Dv=4), "D128": dict(Da=128, Dv=128, cache=TINY),
    "H1": dict(H=1), "H3": dict(H=3), "targets_0": dict(num_targets=[0] * 8), "targets_below_delta": dict(num_targets=[3] * 8),
    "targets_delta": dict(num_targets=[17] * 8), "targets_above_delta": dict(num_targets=[17, 18, 20, 30, 33, 40, 70, 82]), "targets_mixed": dict(num_targets=MIXED),
    "window_1": dict(L=1), "window_16": dict(L=T, num_targets=MIXED), "window_past_a_chunk": dict(L=C + 1, cache=[4 * T, C + 40], num_targets=[3, 17]),
    "contextual_1": dict(c=1), "contextual_3": dict(c=3), "contextual_17": dict(c=T + 1), "contextual_3_targets": dict(c=3, num_targets=MIXED),
    "contextual_17_targets_window": dict(c=T + 1, num_targets=MIXED, L=5), "scaling_seqlen": dict(scaling_seqlen=7),
    "uvqk_slices": dict(sliced=True, num_targets=MIXED), "empty_batch": dict(cache=[]),
    "longer_than_max_seq_len": dict(max_seq_len=4 * T + 17, scaling_seqlen=50, refused=(7,), num_targets=MIXED, c=2),
}


def sliced(dev, k, v, q):
    """v, q, k as the uvqk product leaves them: column slices of one [N, (2 Dv + 2 Da) H] matrix"""
    (N, H, Da), Dv = k.shape, v.shape[2]
    _, c, a, b = torch.split(torch.cat([torch.zeros(N, H * Dv), v.reshape(N, -1), q.reshape(N, -1), k.reshape(N, -1)], dim=1).to(dev), [H * Dv, H * Dv, H * Da, H * Da], dim=1)
    return b.view(N, H, Da), c.view(N, H, Dv), a.view(N, H, Da)


def draw(c, seed):
    """the full sequences (hstu_ref.draw's p), the float64 truth and the float32 gap of the delta rows, the delta rows' indices"""
    lengths, B, d = [n + c["delta"] for n in c["cache"]], len(c["cache"]), c["delta"]
    gen = torch.Generator().manual_seed(seed)
    off = torch.tensor([0] + lengths, dtype=torch.int64).cumsum(0)
    N, msl = int(off[-1]), c["max_seq_len"] or max(lengths + [1])
    p = {"offsets": off, "max_seq_len": max(lengths + [1]), "alpha": c["Da"] ** -0.5, "L": c["L"], "c": c["c"], "max_seq_len_call": msl,
         "scaling_seqlen": c["scaling_seqlen"] if c["scaling_seqlen"] > 0 else msl, "scaling_seqlen_call": c["scaling_seqlen"],
         "num_targets": None if c["num_targets"] is None else torch.tensor(c["num_targets"], dtype=torch.int64),
         "q": torch.randn(N, c["H"], c["Da"], generator=gen), "k": torch.randn(N, c["H"], c["Da"], generator=gen), "v": torch.randn(N, c["H"], c["Dv"], generator=gen)}
    rows = torch.cat([torch.arange(int(off[b + 1]) - d, int(off[b + 1])) for b in range(B)] + [torch.zeros(0, dtype=torch.int64)])
    zero = torch.tensor([b in c["refused"] for b in range(B) for _ in range(d)], dtype=torch.bool).view(-1, 1, 1)
    want, r32 = (ref.attention(p, *(p[x].to(t) for x in "qkv"), t)[rows].masked_fill(zero, 0.0) for t in (torch.float64, torch.float32))
    return p, {"out": [want]}, {"out": ref.rel_err([r32], [want])}, rows


def run(dev, p, c, rows, two_segments, fused=True):
    from torcheasyrec_amd import hstu

    B, d = len(c["cache"]), c["delta"]
    off, k, v = p["offsets"], p["k"], p["v"]
    dq, seg = p["q"][rows], {}
    if two_segments:  # the cached rows packed, the delta rows apart
        keep = torch.ones(k.shape[0], dtype=torch.bool)
        keep[rows] = False
        off, seg = off - d * torch.arange(B + 1), dict(delta_k=k[rows], delta_v=v[rows])
        k, v = k[keep], v[keep]
    if c["sliced"]:
        k, v, _ = sliced(dev, k, v, k)
        if two_segments:
            seg["delta_k"], seg["delta_v"], dq = sliced(dev, seg["delta_k"], seg["delta_v"], dq)
    nt = None if p["num_targets"] is None else p["num_targets"].to(dev)
    before = hstu._HstuDeltaFn.calls
    out = hstu.delta_hstu_mha(p["max_seq_len_call"], p["alpha"], dq.to(dev), k.to(dev), v.to(dev), off.to(dev), num_targets=nt, max_attn_len=p["L"],
                              contextual_seq_len=p["c"], scaling_seqlen=p["scaling_seqlen_call"], **{n: t.to(dev) for n, t in seg.items()})
    assert hstu._HstuDeltaFn.calls == before + (1 if fused else 0)  # (the kernel, or the literal form)
    return {"out": [out.cpu()]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64_in_both_forms(dev, name, monkeypatch):
    from torcheasyrec_amd import hstu

    monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA", True)
    c = {**BASE, **CASES[name]}
    p, want, gaps, rows = draw(c, sorted(CASES).index(name))
    two, one = run(dev, p, c, rows, True), run(dev, p, c, rows, False)
    ref.check(two, want, gaps, f"{name} on {dev.type}", ("out",))
    assert torch.equal(two["out"][0], one["out"][0])
    d = c["delta"]
    assert all(float(two["out"][0][b * d:(b + 1) * d].abs().sum()) == 0.0 for b in c["refused"])


def test_a_full_sequence_shorter_than_delta_gives_zero_rows(dev, monkeypatch):
    from torcheasyrec_amd import hstu

    monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA", True)
    c = {**BASE, "cache": [T, 2], "delta": 5}
    p, want, gaps, rows = draw(c, 200)
    p["offsets"] = torch.tensor([0, T + 5, T + 8])  # the second sample: 3 rows of its own
    for fused in (True, False):
        monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA", fused)
        got = run(dev, p, c, rows, False, fused)
        assert float(got["out"][0][5:].abs().sum()) == 0.0
        ref.check({"out": [got["out"][0][:5]]}, {"out": [want["out"][0][:5]]}, gaps, f"short sample, fused {fused}", ("out",))


def test_two_runs_are_bit_equal(dev, monkeypatch):
    from torcheasyrec_amd import hstu

    monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA", True)
    c = {**BASE, "cache": [3, C + 1, 4 * T], "num_targets": [2, 17, 20], "c": 3, "L": C}
    p, _, _, rows = draw(c, 201)
    assert torch.equal(run(dev, p, c, rows, True)["out"][0], run(dev, p, c, rows, True)["out"][0])


def test_with_the_switch_off_and_outside_the_limits_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import hstu

    assert hstu.delta_hstu_mha_limit(4, 128, 128, 8000, 32) is None and "attention_dim" in hstu.delta_hstu_mha_limit(2, 6, 12, 100, 4) and "delta" in hstu.delta_hstu_mha_limit(2, 8, 12, 100, 0)
    for fused, extra in ((False, dict()), (True, dict(Da=6)), (False, dict(refused=(7,), max_seq_len=4 * T + 17, scaling_seqlen=50))):
        monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA", fused)
        c = {**BASE, "num_targets": MIXED, "c": 3, "L": T + 4, **extra}
        p, want, gaps, rows = draw(c, 202)
        for two in (True, False):
            ref.check(run(dev, p, c, rows, two, fused=False), want, gaps, f"literal {extra} two_segments {two}", ("out",))


LAYER = {
    "targets_below_delta": dict(lengths=[9, 25, 70], delta=8, E=12, H=2, Dv=8, Da=4, num_targets=[0, 3, 7], c=0, L=0, group_norm=False),
    "contextual_all_targets": dict(lengths=[12, 40, 21], delta=5, E=8, H=3, Dv=4, Da=8, num_targets=[5, 5, 5], c=3, L=6, group_norm=True),
}


@pytest.mark.parametrize("name", sorted(LAYER))
def test_a_prefill_and_a_cached_forward_give_the_last_rows_of_the_full_forward(dev, name, monkeypatch):
    from torcheasyrec_amd import hstu

    monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA", True)
    c = LAYER[name]
    d, msl = c["delta"], max(c["lengths"])
    gen = torch.Generator().manual_seed(sorted(LAYER).index(name))
    lengths = torch.tensor(c["lengths"], dtype=torch.int64)
    offsets = torch.cat([lengths.new_zeros(1), lengths.cumsum(0)])
    rows = torch.cat([torch.arange(int(e) - d, int(e)) for e in offsets[1:]])
    nt, x = torch.tensor(c["num_targets"], dtype=torch.int64), torch.randn(int(offsets[-1]), c["E"], generator=gen)
    layers = [hstu.STULayer(c["E"], c["H"], c["Dv"], c["Da"], output_dropout_ratio=0.0, max_attn_len=c["L"], contextual_seq_len=c["c"],
                            use_group_norm=c["group_norm"]) for _ in range(2)]
    for layer in layers:  # every parameter off its constant start
        for t in layer.parameters():
            t.data.add_(0.1 * torch.randn(t.shape, generator=gen))
    p = {"offsets": offsets, "max_seq_len": msl, "L": c["L"], "c": c["c"], "scaling_seqlen": -1, "num_targets": nt}
    ys = {}
    for dtype in (torch.float64, torch.float32):  # the truth and the yardstick: the same stack restated on the CPU
        y = x.to(dtype)
        for layer in layers:
            y = layer_ref(y, [getattr(layer, n).detach().to(dtype) for n in NAMES], p, c, dtype)
        ys[dtype] = [y[rows]]
    stack = hstu.STUStack(layers).to(dev).eval()
    before = hstu._HstuDeltaFn.calls
    with torch.no_grad():
        full = stack(x.to(dev), offsets.to(dev), msl, nt.to(dev), max_kv_caching_len=msl - d, kv_caching_lengths=(lengths - d).to(dev))
        got = stack.cached_forward(x[rows].to(dev), nt.to(dev))
    assert hstu._HstuDeltaFn.calls == before + 2  # each layer took the delta kernel exactly once
    gaps = {"out": ref.rel_err(ys[torch.float32], ys[torch.float64])}
    ref.check({"out": [got.cpu()]}, {"out": ys[torch.float64]}, gaps, f"{name} cached on {dev.type}", ("out",))
    ref.check({"out": [full[rows.to(dev)].cpu()]}, {"out": ys[torch.float64]}, gaps, f"{name} full on {dev.type}", ("out",))
