"""hstu.delta_hstu_mha on bf16 operands (tzr_hstu_delta_bf16_fwd, csrc/hstu_delta_bf16.hip) and a bf16 STUStack.cached_forward,
on the cases and through the `run` of tests/test_hstu_delta.py.  The truth is hstu_ref.attention in float64 on the FULL sequences,
computed from the bf16-rounded values the kernel sees, of which each sample's last `delta` rows are compared: max |got - fp64| /
max(1, |fp64|) at or below 4 x the distance of the same dense form run in bf16, floor 2^-20.  Every case runs in the two-segment and
in the one-segment form, and the two are bit-equal.  The cache lengths sit on the edges of the kernel's 32-key tiles, of the four
waves' share (4 tiles) and of its HSTU_DELTA_CHUNK-key chunks."""
import ctypes as C
import os

import pytest
import torch

import hstu_ref as ref
import test_hstu_delta as hd
from test_stu_layer import NAMES, layer_ref
from torcheasyrec_amd import _lib

BF = torch.bfloat16
T, CH = _lib.HSTU_BF16_TILE, _lib.HSTU_DELTA_CHUNK
SHORT = [0, 1, T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1]
MIXED = [0, 1, 3, 17, 18, 40, 2, 17]  # targets per sample of SHORT at delta 17: none, below, equal to and above delta
BASE = {**hd.BASE, "cache": SHORT, "Da": 8, "Dv": 16}
CASES = {
    "chunk_edges": dict(cache=[CH - 1, CH, CH + 1, 2 * CH + 1]), "delta_1": dict(delta=1), "delta_15": dict(delta=15), "delta_16": dict(delta=16),
    "delta_33": dict(delta=33, num_targets=[33] * 8), "Da24_Dv8": dict(Da=24, Dv=8), "Da40_Dv24": dict(Da=40, Dv=24), "D128": dict(Da=128, Dv=128, cache=hd.TINY),
    "H1": dict(H=1), "H3": dict(H=3), "targets_mixed": dict(num_targets=MIXED), "window_1": dict(L=1), "window_36": dict(L=T + 4, num_targets=MIXED),
    "window_past_a_chunk": dict(L=CH + 1, cache=[4 * T, CH + 40], num_targets=[3, 17]), "contextual_3": dict(c=3), "contextual_33": dict(c=T + 1),
    "contextual_3_targets_window": dict(c=3, num_targets=MIXED, L=5), "contextual_33_targets_window": dict(c=T + 1, num_targets=MIXED, L=5),
    "scaling_seqlen": dict(scaling_seqlen=7), "uvqk_slices": dict(sliced=True, num_targets=MIXED), "empty_batch": dict(cache=[]),
    "longer_than_max_seq_len": dict(max_seq_len=4 * T + 17, scaling_seqlen=50, refused=(7,), num_targets=MIXED, c=2),
}
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


def draw(c, seed):
    """hd.draw with q, k, v rounded to bf16 (p holds them as bf16): the float64 truth and the bf16 gap of the delta rows"""
    lengths, B, d = [n + c["delta"] for n in c["cache"]], len(c["cache"]), c["delta"]
    gen = torch.Generator().manual_seed(seed)
    off = torch.tensor([0] + lengths, dtype=torch.int64).cumsum(0)
    N, msl = int(off[-1]), c["max_seq_len"] or max(lengths + [1])
    p = {"offsets": off, "max_seq_len": max(lengths + [1]), "alpha": c["Da"] ** -0.5, "L": c["L"], "c": c["c"], "max_seq_len_call": msl,
         "scaling_seqlen": c["scaling_seqlen"] if c["scaling_seqlen"] > 0 else msl, "scaling_seqlen_call": c["scaling_seqlen"],
         "num_targets": None if c["num_targets"] is None else torch.tensor(c["num_targets"], dtype=torch.int64),
         **{x: torch.randn(N, c["H"], c[w], generator=gen).to(BF) for x, w in (("q", "Da"), ("k", "Da"), ("v", "Dv"))}}
    rows = torch.cat([torch.arange(int(off[b + 1]) - d, int(off[b + 1])) for b in range(B)] + [torch.zeros(0, dtype=torch.int64)])
    zero = torch.tensor([b in c["refused"] for b in range(B) for _ in range(d)], dtype=torch.bool).view(-1, 1, 1)
    want, lit = (ref.attention(p, *(p[x].to(t) for x in "qkv"), t)[rows].masked_fill(zero, 0.0) for t in (torch.float64, BF))
    return p, {"out": [want]}, {"out": ref.rel_err([lit.double()], [want])}, rows


def sliced(dev, k, v, q):
    """hd.sliced in the operands' dtype: column slices of one bf16 uvqk matrix"""
    (N, H, Da), Dv = k.shape, v.shape[2]
    _, c, a, b = torch.split(torch.cat([v.new_zeros(N, H * Dv), v.reshape(N, -1), q.reshape(N, -1), k.reshape(N, -1)], dim=1).to(dev), [H * Dv, H * Dv, H * Da, H * Da], dim=1)
    return b.view(N, H, Da), c.view(N, H, Dv), a.view(N, H, Da)


@pytest.fixture
def switches(monkeypatch):
    from torcheasyrec_amd import hstu

    monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA", True)
    monkeypatch.setattr(hstu, "FUSED_HSTU_DELTA_BF16", True)
    monkeypatch.setattr(hd, "sliced", sliced)
    return monkeypatch


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64_in_both_forms(dev, name, switches):
    c = {**BASE, **CASES[name]}
    p, want, gaps, rows = draw(c, sorted(CASES).index(name))
    two, one = hd.run(dev, p, c, rows, True), hd.run(dev, p, c, rows, False)  # (asserts that each call took the kernel)
    assert two["out"][0].dtype == BF and one["out"][0].dtype == BF
    ref.check(two, want, gaps, f"{name} on {dev.type}", ("out",))
    assert torch.equal(two["out"][0], one["out"][0])
    d = c["delta"]
    assert all(float(two["out"][0][b * d:(b + 1) * d].abs().sum()) == 0.0 for b in c["refused"])


def test_two_runs_are_bit_equal(dev, switches):
    c = {**BASE, "cache": [3, CH + 1, 4 * T], "num_targets": [2, 17, 20], "c": 3, "L": CH}
    p, _, _, rows = draw(c, 201)
    assert torch.equal(hd.run(dev, p, c, rows, True)["out"][0], hd.run(dev, p, c, rows, True)["out"][0])


def test_switch_off_outside_the_limits_and_mixed_dtypes_take_the_literal_form_and_fp32_its_own_kernel(dev, switches):
    from torcheasyrec_amd import hstu

    assert hstu.delta_hstu_mha_limit(4, 128, 128, 8000, 32, dtype=BF) is None and "attention_dim" in hstu.delta_hstu_mha_limit(2, 12, 16, 100, 4, dtype=BF)
    assert hstu.delta_hstu_mha_limit(2, 12, 16, 100, 4) is None
    for off, extra, mixed in ((True, dict(), False), (False, dict(Da=12), False), (False, dict(), True)):
        switches.setattr(hstu, "FUSED_HSTU_DELTA_BF16", not off)
        c = {**BASE, "num_targets": MIXED, "c": 3, "L": T + 4, **extra}
        p, want, gaps, rows = draw(c, 202)
        if mixed:  # bf16 delta_q against fp32 keys and values
            p["k"], p["v"] = p["k"].float(), p["v"].float()
        for two in (True, False):
            ref.check(hd.run(dev, p, c, rows, two, fused=False), want, gaps, f"literal off {off} {extra} mixed {mixed} two_segments {two}", ("out",))
    for x in "qkv":  # fp32 operands: the fp32 kernel (`run` counts the call), an fp32 result
        p[x] = p[x].float()
    assert hd.run(dev, p, c, rows, True)["out"][0].dtype == torch.float32


BOUNDARY = {
    "valid_but_empty_batch": (dict(B=0, delta_q=0, k=0, v=0, k_delta=0, v_delta=0, out=0, offsets=0), OK), "width_4": (dict(Da=4), UNSUPPORTED),
    "k_8_bytes_off": (dict(k="+8"), INVALID), "v_delta_stride_4_elements_off": (dict(v_delta_stride="+4"), UNSUPPORTED),
    "two_chunks_without_a_workspace": (dict(max_seq_len=CH + 1), WORKSPACE),
}


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_the_c_boundary(dev, name):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    assert "tzr_hstu_delta_bf16_fwd" in _lib.EXPORTED_SYMBOLS and " tzr_hstu_delta_bf16_fwd(" in header and C.sizeof(_lib.TzrHstuDelta) == 232
    fields, code = BOUNDARY[name]
    B, d, H, Da, Dv = 2, 3, 2, 8, 16
    keep = {x: torch.zeros(n, H, 24, dtype=BF, device=dev) for x, n in (("delta_q", B * d), ("k", 9), ("v", 9), ("k_delta", B * d), ("v_delta", B * d), ("out", B * d))}
    off = torch.tensor([0, 4, 9], dtype=torch.int64).to(dev)
    m = _lib.TzrHstuDelta()
    m.B, m.Nc, m.H, m.Da, m.Dv, m.delta, m.max_seq_len, m.scaling_seqlen, m.alpha, m.offsets = B, 9, H, Da, Dv, d, 16, -1, 0.3, off.data_ptr()
    for x, t in keep.items():
        setattr(m, x, t.data_ptr()), setattr(m, x + "_stride", t.stride(0)), setattr(m, x + "_head_stride", t.stride(1))
    for k, v in fields.items():
        setattr(m, k, getattr(m, k) + int(v) if isinstance(v, str) else v)
    L = _lib.lib()
    assert L.tzr_hstu_delta_bf16_fwd(None, None) == INVALID and L.tzr_hstu_delta_bf16_fwd(C.byref(m), _lib.stream_ptr(dev)) == code


def test_a_bf16_stack_prefills_a_bf16_cache_and_serves_from_it_on_the_kernel(dev, switches):
    """two STU layers cast to bf16 (`contextual_all_targets` of hd.LAYER with Dv raised to 8: the bf16 kernels take multiples of 8):
    the cached rows against the float64 stack on the bf16-rounded weights; the yardstick is the same bf16 stack with the switch off"""
    from torcheasyrec_amd import hstu

    c = {**hd.LAYER["contextual_all_targets"], "Dv": 8}
    d, msl = c["delta"], max(c["lengths"])
    gen = torch.Generator().manual_seed(3)
    lengths = torch.tensor(c["lengths"], dtype=torch.int64)
    offsets = torch.cat([lengths.new_zeros(1), lengths.cumsum(0)])
    rows = torch.cat([torch.arange(int(e) - d, int(e)) for e in offsets[1:]])
    nt, x = torch.tensor(c["num_targets"], dtype=torch.int64), torch.randn(int(offsets[-1]), c["E"], generator=gen).to(BF)
    layers = [hstu.STULayer(c["E"], c["H"], c["Dv"], c["Da"], output_dropout_ratio=0.0, max_attn_len=c["L"], contextual_seq_len=c["c"], use_group_norm=True) for _ in range(2)]
    for layer in layers:  # every parameter off its constant start
        for t in layer.parameters():
            t.data.add_(0.1 * torch.randn(t.shape, generator=gen))
    stack = hstu.STUStack(layers).to(dev).to(BF).eval()
    p = {"offsets": offsets, "max_seq_len": msl, "L": c["L"], "c": c["c"], "scaling_seqlen": -1, "num_targets": nt}
    y = x.double()
    for layer in layers:
        y = layer_ref(y, [getattr(layer, n).detach().cpu().double() for n in NAMES], p, c, torch.float64)

    def go(calls):
        before = hstu._HstuDeltaFn.calls
        with torch.no_grad():
            stack(x.to(dev), offsets.to(dev), msl, nt.to(dev), max_kv_caching_len=msl - d, kv_caching_lengths=(lengths - d).to(dev))
            got = stack.cached_forward(x[rows].to(dev), nt.to(dev))
        assert hstu._HstuDeltaFn.calls == before + calls and all(layer.k_cache.dtype == BF for layer in layers) and got.dtype == BF
        return [got.cpu().double()]

    got = go(2)  # each layer took the delta kernel exactly once
    switches.setattr(hstu, "FUSED_HSTU_DELTA_BF16", False)
    ref.check({"out": got}, {"out": [y[rows]]}, {"out": ref.rel_err(go(0), [y[rows]])}, f"bf16 cached stack on {dev.type}", ("out",))
