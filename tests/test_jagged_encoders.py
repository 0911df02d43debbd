"""The two cheap sequence encoders (sequence.SimpleAttention, sequence.PoolingEncoder) and their jagged kernels
(csrc/jagged_encoders.hip).

* Both evaluations of both encoders -- the padded torch form on `<g>.sequence`, the jagged form on the same rows without
  padding -- against vectors the REFERENCE's own modules produced (tests/golden/make_reference_seq_encoder_vectors.py):
  outputs and input gradients, rtol = atol = 1e-5 (what tests/test_sequence_parity.py holds the jagged DIN tower to; the sums
  here are shorter: at most 8 positions of 48 columns).
* The kernels' edge cases against the padded restatement of tests/seq_encoder_ref.py evaluated in float64 (so the figure
  compared against carries no rounding of its own), same tolerance: inputs are drawn at a scale that keeps the attention
  scores O(1) and a sample's |row| sums below ~300, so a sum of n <= 1100 fp32 terms added group-wise (at most n / G + 6
  additions deep, G >= 1 groups) stays some 1e-6 from the exact one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import seq_encoder_ref as ref  # noqa: E402
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.sequence import PoolingEncoder, SimpleAttention, jagged_dot_attention, jagged_pool  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_VEC = {}


def _vectors():
    if not _VEC:
        _VEC.update(np.load(os.path.join(HERE, "golden", "reference_seq_encoder_vectors.npz")))
    return _VEC


def _offsets(lengths):
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64), 0)
    return off


@pytest.mark.parametrize("form", ["padded", "jagged"])
@pytest.mark.parametrize("msl", [0, 6])
@pytest.mark.parametrize("D", [16, 48])
@pytest.mark.parametrize("kind", ["attn", "sum", "mean"])
def test_encoders_match_the_reference_modules(dev, kind, D, msl, form):
    v = _vectors()
    tag = f"{kind}_d{D}_m{msl}"
    q0, s0, ln = torch.from_numpy(v[f"{tag}/query"]), torch.from_numpy(v[f"{tag}/sequence"]), torch.from_numpy(v[f"{tag}/length"])
    B, L, _ = s0.shape
    enc = SimpleAttention(D, D, "g", max_seq_length=msl) if kind == "attn" else PoolingEncoder(D, "g", pooling_type=kind, max_seq_length=msl)
    assert enc.input() == "g" and enc.output_dim() == D
    q = q0.clone().to(dev).requires_grad_(True)
    valid = (torch.arange(L).unsqueeze(0) < ln.unsqueeze(1))
    if form == "padded":
        s = s0.clone().to(dev).requires_grad_(True)
        y = enc({"g.query": q, "g.sequence": s, "g.sequence_length": ln.to(dev)})
    else:  # the same rows without the padding
        s = s0[valid].clone().to(dev).requires_grad_(True)
        assert s.shape[0] == int(ln.sum())
        y = enc({"g.query": q, "g.sequence_jagged": s, "g.sequence_offsets": _offsets(ln).to(dev), "g.sequence_max_len": L,
                 "g.sequence_length": ln.to(dev)})
    y.backward(torch.from_numpy(v[f"{tag}/gy"]).to(dev))
    torch.testing.assert_close(y.detach().cpu(), torch.from_numpy(v[f"{tag}/y"]), rtol=1e-5, atol=1e-5)
    gs = torch.from_numpy(v[f"{tag}/gsequence"])
    torch.testing.assert_close(s.grad.cpu(), gs if form == "padded" else gs[valid], rtol=1e-5, atol=1e-5)
    if kind == "attn":
        torch.testing.assert_close(q.grad.cpu(), torch.from_numpy(v[f"{tag}/gquery"]), rtol=1e-5, atol=1e-5)
    assert bool((y.detach()[0] == 0).all())  # the sample without a position


def test_simple_attention_refuses_unequal_dims_at_construction():
    with pytest.raises(ValueError, match="query_dim"):
        SimpleAttention(16, 12, "g")


# (D, lengths, max_len): D = 4 and 256 (one lane / all 64 lanes per row), 48 (12 of a group's 16 lanes hold a piece); one sample of
# 70 positions (more than a wave's 64 lanes: the loops over a sample's scores wrap); samples at, one over and far over what a
# wave holds in registers between its two passes (16 * 64 / P positions: 1024 at D = 4, 64 at D = 48, 16 at D = 256); a sample
# longer than max_len; B = 1; a batch without any position
CASES = {
    "d4": (4, [70, 0, 3, 1100, 1], 2048),
    "d256": (256, [70, 0, 3, 16, 17, 1], 100),
    "d48_hold": (48, [64, 65, 0, 1, 9], 80),
    "truncated": (16, [12, 5, 0, 9, 7, 8], 7),
    "one_sample": (16, [5], 8),
    "all_empty": (16, [0, 0, 0], 8),
}
_REF = {}


def _case(name):
    """inputs and the float64 padded restatement's outputs and gradients, computed once per case"""
    if name not in _REF:
        D, lengths, max_len = CASES[name]
        g = torch.Generator().manual_seed(len(name) * 100 + D)
        N, B = sum(lengths), len(lengths)
        rows = torch.randn(N, D, generator=g) * (0.25 if D <= 16 else D ** -0.5)
        query = torch.randn(B, D, generator=g) * (2.0 if D <= 16 else 4.0)
        gy = torch.randn(B, D, generator=g)
        L = min(max(lengths + [1]), max_len)
        want = {}
        for kind in ("attn", "sum", "mean"):
            r, q = rows.double().requires_grad_(True), query.double().requires_grad_(True)
            y = ref.simple_attention(q, r, lengths, L) if kind == "attn" else ref.pooling(r, lengths, L, kind)
            (y * gy.double()).sum().backward()
            want[kind] = (y.detach().float(), r.grad.float(), q.grad.float() if kind == "attn" else None)
        _REF[name] = (rows, query, gy, want)
    return _REF[name]


def _run(dev, kind, rows, query, gy, lengths, max_len):
    r, q = rows.clone().to(dev).requires_grad_(True), query.clone().to(dev).requires_grad_(True)
    off = _offsets(lengths).to(dev)
    y = jagged_dot_attention(r, q, off, max_len) if kind == "attn" else jagged_pool(r, off, max_len, kind)
    (y * gy.to(dev)).sum().backward()
    return y.detach().cpu(), r.grad.cpu(), q.grad.cpu() if kind == "attn" else None


@pytest.mark.parametrize("kind", ["attn", "sum", "mean"])
@pytest.mark.parametrize("name", list(CASES))
def test_jagged_kernels_edge_cases(dev, name, kind):
    D, lengths, max_len = CASES[name]
    rows, query, gy, want = _case(name)
    got = _run(dev, kind, rows, query, gy, lengths, max_len)
    again = _run(dev, kind, rows, query, gy, lengths, max_len)
    for what, a, b, w in zip(("out", "d rows", "d query"), got, again, want[kind]):
        if a is None:
            continue
        assert torch.equal(a, b), f"{what}: two runs differ"  # fixed summation order, no atomics
        torch.testing.assert_close(a, w, rtol=1e-5, atol=1e-5, msg=lambda m, what=what: f"{what}: {m}")
    assert tuple(got[0].shape) == (len(lengths), D) and tuple(got[1].shape) == (sum(lengths), D)
    # positions at or behind max_len: rows of exact zeros in the gradient; samples without a position: a zero output row
    off = _offsets(lengths)
    for b, n in enumerate(lengths):
        if n > max_len:
            assert bool((got[1][int(off[b]) + max_len:int(off[b + 1])] == 0).all())
        if n == 0:
            assert bool((got[0][b] == 0).all()) and (kind != "attn" or bool((got[2][b] == 0).all()))


@pytest.mark.parametrize("kind", ["attn", "mean"])
def test_rows_taken_as_a_column_slice_of_a_wider_tensor(dev, kind):
    """non-contiguous strides reach the kernels as they are (row stride 40 floats, first column 4 floats in): same bits as
    the contiguous copy"""
    from torcheasyrec_amd._lib import rows16 as _rows

    D, lengths, max_len = 32, [9, 0, 70, 3], 80
    g = torch.Generator().manual_seed(9)
    wide_r, wide_q, wide_g = (torch.randn(n, D + 8, generator=g).to(dev) * 0.25 for n in (sum(lengths), len(lengths), len(lengths)))
    off = _offsets(lengths).to(dev)
    res = []
    for contiguous in (False, True):
        r, q, gy = (w[:, 4:4 + D] for w in (wide_r, wide_q, wide_g))
        assert _rows(r) is r and r.stride(0) == D + 8
        if contiguous:
            r, q, gy = r.contiguous(), q.contiguous(), gy.contiguous()
        r, q = r.detach().requires_grad_(True), q.detach().requires_grad_(True)
        y = jagged_dot_attention(r, q, off, max_len) if kind == "attn" else jagged_pool(r, off, max_len, kind)
        y.backward(gy)
        res.append([y.detach().cpu(), r.grad.cpu()] + ([q.grad.cpu()] if kind == "attn" else []))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][0].abs().sum()) > 0


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("kind", ["attn", "mean"])
def test_one_row_slices_of_a_wider_tensor(dev, kind, N):
    """B = 1, N = 1: rows, query and output gradient are one-row slices [1:2, :8] of [4, 10] tensors -- row stride 10 floats, first
    float 8 bytes past a 16-byte boundary, and "contiguous" to torch whatever their strides, so .contiguous() hands them on as they
    are and the library refuses them (TZR_ERR_UNSUPPORTED: the row stride).  The encoders copy such rows (`_lib.rows16` clones).
    N = 2: the one-row query and output gradient beside two rows -- over one score the softmax is 1 whatever the query holds; over
    two, the copy of the query is what the outputs and gradients show."""
    D, lengths, max_len = 8, [N], 4
    g = torch.Generator().manual_seed(11)
    rows, query, gy = (torch.randn(4, D + 2, generator=g).to(dev)[1:1 + n, :D] for n in (N, 1, 1))
    assert query.contiguous().data_ptr() == query.data_ptr() and gy.data_ptr() % 16 == 8
    assert N > 1 or rows.contiguous().data_ptr() == rows.data_ptr() and rows.data_ptr() % 16 == 8 and rows.stride(0) == D + 2
    r, q = rows.detach().requires_grad_(True), query.detach().requires_grad_(True)
    y = jagged_dot_attention(r, q, _offsets(lengths).to(dev), max_len) if kind == "attn" else jagged_pool(r, _offsets(lengths).to(dev), max_len, kind)
    y.backward(gy)
    rd, qd = rows.detach().cpu().double().requires_grad_(True), query.detach().cpu().double().requires_grad_(True)
    want = ref.simple_attention(qd, rd, lengths, N) if kind == "attn" else ref.pooling(rd, lengths, N, kind)
    want.backward(gy.cpu().double())
    torch.testing.assert_close(y.detach().cpu(), want.detach().float(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(r.grad.cpu(), rd.grad.float(), rtol=1e-5, atol=1e-5)
    if kind == "attn":
        torch.testing.assert_close(q.grad.cpu(), qd.grad.float(), rtol=1e-5, atol=1e-5)


def test_max_len_bound_of_the_attention_kernels(dev):
    """a sample's scores live in LDS: max_len = 2048 is taken, 2049 refused (the pooling kernels keep nothing: any max_len)"""
    L, p = _lib.lib(), _lib.ptr
    D, B, N = 8, 2, 5
    kv, q, out, pr, dkv, dq = (torch.zeros(n, dtype=torch.float32, device=dev) for n in (N * D, B * D, B * D, N, N * D, B * D))
    off = torch.tensor([0, 2, 5], dtype=torch.int64, device=dev)
    for max_len, rc in ((2048, 0), (2049, -4)):
        assert L.tzr_jagged_dot_attn_fwd(p(kv), D, p(q), D, D, p(off), B, N, max_len, p(out), D, p(pr), None) == rc
        assert L.tzr_jagged_dot_attn_bwd(p(out), D, p(pr), p(kv), D, p(q), D, D, p(off), B, N, max_len, p(dkv), D, p(dq), D, None) == rc
    assert L.tzr_jagged_pool_fwd(p(kv), D, D, p(off), B, N, 1 << 40, 1, p(out), D, None) == 0
    assert L.tzr_jagged_pool_bwd(p(out), D, D, p(off), B, N, 1 << 40, 1, p(dkv), D, None) == 0
    with pytest.raises(ValueError, match="max_len"):
        SimpleAttention(D, D, "g")({"g.query": q.view(B, D), "g.sequence_jagged": kv.view(N, D), "g.sequence_offsets": off,
                                    "g.sequence_max_len": 2049})
