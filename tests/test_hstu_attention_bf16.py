"""hstu.hstu_mha on bf16 q, k, v (tzr_hstu_attn_bf16_fwd / _bwd, csrc/hstu_attention_bf16.hip) against the per-sample dense form in
float64 on the CPU (tests/hstu_ref.py) computed from the bf16-rounded values the kernel sees: the output and dq, dk, dv under a
random upstream gradient.  Per kind: max |got - fp64| / max(1, |fp64|) at or below 4 x the distance of the same dense form run in
bf16, floor 2^-20.  The lengths sit on the edges of the kernels' HSTU_BF16_BLOCK-row blocks and HSTU_BF16_TILE-key tiles."""
import ctypes as C
import os

import pytest
import torch

import hstu_ref as ref
from torcheasyrec_amd import _lib

BF = torch.bfloat16
BLK, TILE = _lib.HSTU_BF16_BLOCK, _lib.HSTU_BF16_TILE
EDGES = [0, 1, TILE - 1, TILE, TILE + 1, BLK - 1, BLK, BLK + 1, 2 * BLK + 1]
SHORT = [0, 1, TILE + 1, 5]  # (the 128-wide cases: the emulator's sake)
MIXED = [0, 0, 3, TILE, 1, 0, 40, TILE + 1, 2 * BLK + 1]  # targets per sample of EDGES, one equal to n, one crossing a tile
BASE = dict(lengths=EDGES, H=2, Da=8, Dv=16, max_seq_len=2 * BLK + 8, num_targets=None, L=0, c=0, sliced=False)
CASES = {
    "base": dict(), "Da24": dict(Da=24), "Da32": dict(Da=32), "Da40": dict(Da=40), "Da128": dict(Da=128, lengths=SHORT),
    "Dv128": dict(Dv=128, lengths=SHORT), "Dv8": dict(Dv=8), "Dv24": dict(Dv=24), "H1": dict(H=1), "H3": dict(H=3),
    "targets_mixed": dict(num_targets=MIXED), "contextual_33_targets": dict(c=TILE + 1, num_targets=MIXED), "window_36": dict(L=TILE + 4),
    "all_three": dict(num_targets=MIXED, c=TILE + 1, L=TILE + 4),
    "longer_than_max_seq_len": dict(lengths=[BLK + 9, 3, TILE + 2, 2 * BLK], max_seq_len=BLK + 1, num_targets=[2, 0, 1, 70], c=2),
    "uvqk_slices": dict(sliced=True, num_targets=MIXED), "empty_batch": dict(lengths=[]),
}
OK, INVALID, UNSUPPORTED = 0, -1, -4


def draw(name_or_seed, **over):
    """ref.draw with q, k, v, g rounded to bf16 and back: the truth is computed from the values the kernel sees"""
    c = {**BASE, **(CASES[name_or_seed] if isinstance(name_or_seed, str) else {}), **over}
    seed = sorted(CASES).index(name_or_seed) if isinstance(name_or_seed, str) else name_or_seed
    p, _ = ref.draw(c["lengths"], c["H"], c["Da"], c["Dv"], c["max_seq_len"], seed, c["num_targets"], c["L"], c["c"])
    for x in "qkvg":
        p[x] = p[x].to(BF).float()
    want = ref.literal(p)
    lit = ref.literal(p, BF)
    return c, p, want, {k: ref.rel_err([t.double() for t in lit[k]], want[k]) for k in ref.KINDS}


def run(dev, p, sliced=False, fused=True):
    from torcheasyrec_amd import hstu

    q, k, v = (p[x].to(dev, BF).requires_grad_(True) for x in "qkv")
    a, b, c = q, k, v
    if sliced:  # u, v, q, k as a bf16 uvqk product leaves them: column slices of one [N, (2 Dv + 2 Da) H] matrix
        (N, H, Da), Dv = q.shape, v.shape[2]
        u = torch.zeros(N, H * Dv, device=dev, dtype=BF)
        _, c, a, b = torch.split(torch.cat([u, v.reshape(N, -1), q.reshape(N, -1), k.reshape(N, -1)], dim=1), [H * Dv, H * Dv, H * Da, H * Da], dim=1)
        a, b, c = a.view(N, H, Da), b.view(N, H, Da), c.view(N, H, Dv)
    nt = None if p["num_targets"] is None else p["num_targets"].to(dev)
    before = hstu._HstuMhaFn.calls
    out = hstu.hstu_mha(p["max_seq_len"], p["alpha"], a, b, c, p["offsets"].to(dev), num_targets=nt, max_attn_len=p["L"], contextual_seq_len=p["c"])
    assert hstu._HstuMhaFn.calls == before + (1 if fused else 0)  # (the bf16 kernels, or the literal form)
    dq, dk, dv = torch.autograd.grad((out.float() * p["g"].to(dev)).sum(), [q, k, v])
    assert all(t.dtype == BF for t in (out, dq, dk, dv))
    return {"out": [out.detach().double()], "dq": [dq.double()], "dk": [dk.double()], "dv": [dv.double()]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64(dev, name):
    c, p, want, gaps = draw(name)
    got = run(dev, p, c["sliced"])
    ref.check(got, want, gaps, f"{name} on {dev.type}", ref.KINDS)
    offsets = p["offsets"].tolist()
    for b, n in enumerate(c["lengths"]):  # rows behind max_seq_len: zero output, zero gradients
        behind = slice(offsets[b] + min(n, c["max_seq_len"]), offsets[b + 1])
        assert all(float(got[k][0][behind].abs().sum()) == 0.0 for k in ref.KINDS)


def test_two_runs_are_bit_equal(dev):
    _, p, _, _ = draw(100, num_targets=MIXED, L=TILE + 4, c=3)
    a, b = run(dev, p), run(dev, p)
    assert all(torch.equal(a[k][0], b[k][0]) for k in ref.KINDS)


def test_outside_the_limits_and_with_the_switch_off_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import hstu

    assert hstu.hstu_mha_limit(4, 128, 128, 8000, dtype=BF) is None and "attention_dim" in hstu.hstu_mha_limit(2, 12, 16, 100, dtype=BF)
    assert hstu.hstu_mha_limit(2, 12, 16, 100) is None and "dtype" in hstu.hstu_mha_limit(2, 8, 8, 100, dtype=torch.float16)
    _, p, want, gaps = draw(101, Da=12, lengths=SHORT)  # Da = 12: a multiple of 4, not of 8
    ref.check(run(dev, p, fused=False), want, gaps, "literal Da 12", ref.KINDS)
    monkeypatch.setattr(hstu, "FUSED_HSTU_MHA_BF16", False)
    _, p, want, gaps = draw(102, lengths=SHORT)
    ref.check(run(dev, p, fused=False), want, gaps, "switch off", ref.KINDS)


BOUNDARY = {
    "valid_but_empty_batch": (dict(B=0, q=0, k=0, v=0, out=0, grad_out=0, dq=0, dk=0, dv=0, offsets=0), OK),
    "q_null": (dict(q=0), INVALID), "width_4": (dict(Da=4), UNSUPPORTED), "k_8_bytes_off": (dict(k="+8"), INVALID),
    "q_stride_4_elements_off": (dict(q_stride="+4"), UNSUPPORTED),
}


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_the_c_boundary(dev, name):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "tzrec_hip.h")).read()
    for sym in ("tzr_hstu_attn_bf16_fwd", "tzr_hstu_attn_bf16_bwd"):
        assert sym in _lib.EXPORTED_SYMBOLS and f" {sym}(" in header
    assert C.sizeof(_lib.TzrHstuAttn) == 264 and f"#define TZR_HSTU_BF16_BLOCK {BLK}\n" in header and f"#define TZR_HSTU_BF16_TILE {TILE}\n" in header
    fields, code = BOUNDARY[name]
    N, H, Da, Dv = 8, 2, 8, 16
    keep = {x: torch.zeros(N, H, 24, dtype=BF, device=dev) for x in ("q", "k", "v", "out", "grad_out", "dq", "dk", "dv")}
    off = torch.tensor([0, 3, N], dtype=torch.int64).to(dev)
    m = _lib.TzrHstuAttn()
    m.B, m.N, m.H, m.Da, m.Dv, m.max_seq_len, m.scaling_seqlen, m.alpha, m.offsets = 2, N, H, Da, Dv, 16, -1, 0.3, off.data_ptr()
    for x, t in keep.items():
        setattr(m, x, t.data_ptr()), setattr(m, x + "_stride", t.stride(0)), setattr(m, x + "_head_stride", t.stride(1))
    for k, v in fields.items():
        setattr(m, k, getattr(m, k) + int(v) if isinstance(v, str) else v)
    L = _lib.lib()
    assert L.tzr_hstu_attn_bf16_fwd(None, None) == INVALID and L.tzr_hstu_attn_bf16_bwd(None, None) == INVALID
    assert L.tzr_hstu_attn_bf16_fwd(C.byref(m), _lib.stream_ptr(dev)) == code and L.tzr_hstu_attn_bf16_bwd(C.byref(m), _lib.stream_ptr(dev)) == code


def test_a_bf16_stack_takes_the_kernel(dev, monkeypatch):
    """two STU layers cast to bf16 (the `group_norm` shape of tests/test_stu_layer.py, with Dv and Da raised to 8: the bf16 kernel
    takes multiples of 8) against the float64 stack on the bf16-rounded weights; the yardstick is the same stack with the switch off"""
    from test_stu_layer import NAMES, SHAPES, stack_ref
    from torcheasyrec_amd import hstu

    c = {**SHAPES["group_norm"], "Dv": 8, "Da": 8}
    gen = torch.Generator().manual_seed(7)
    offsets = torch.tensor([0] + c["lengths"], dtype=torch.int64).cumsum(0)
    N = int(offsets[-1])
    x, g = torch.randn(N, c["E"], generator=gen).to(BF), torch.randn(N, c["E"], generator=gen)
    layers = [hstu.STULayer(c["E"], c["H"], c["Dv"], c["Da"], output_dropout_ratio=0.0, max_attn_len=c["L"], use_group_norm=True) for _ in range(2)]
    for layer in layers:
        for t in layer.parameters():
            t.data.add_(0.1 * torch.randn(t.shape, generator=gen))
    stack = hstu.STUStack(layers).to(dev).to(BF)
    p = {"offsets": offsets, "max_seq_len": c["max_seq_len"], "L": c["L"], "c": 0, "scaling_seqlen": -1, "num_targets": None}
    want = stack_ref(x.double(), [[getattr(layer, n) for n in NAMES] for layer in layers], g, p, c, torch.float64)
    want = {"out": want["out"], "dx": want["grads"][:1]}

    def go(calls):
        xd = x.to(dev).requires_grad_(True)
        before = hstu._HstuMhaFn.calls
        out = stack(xd, offsets.to(dev), c["max_seq_len"])
        assert hstu._HstuMhaFn.calls == before + calls and out.dtype == BF
        return {"out": [out.detach().double()], "dx": [torch.autograd.grad((out.float() * g.to(dev)).sum(), xd)[0].double()]}

    got = go(2)
    monkeypatch.setattr(hstu, "FUSED_HSTU_MHA_BF16", False)
    lit = go(0)
    ref.check(got, want, {k: ref.rel_err(lit[k], want[k]) for k in want}, f"bf16 stack on {dev.type}", ("out", "dx"))
