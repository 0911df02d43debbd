"""Jagged <-> padded dense and segment reduce (csrc/jagged_ops.hip) where their loops run more than once: truncated tails of
thousands of float4, more work than the capped grid covers at once, rows inside wider buffers (`values_stride > dim`),
`max_len == 0`, segments of hundreds of rows.  The copies are compared bit-exactly with the oracle and its autograd, the
reductions with torch.segment_reduce in float64 under the bound of an in-order fp32 sum.  tests/test_sequence_parity.py holds
the small shapes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle import tzrec_oracle as orc  # noqa: E402
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.sequence import jagged_to_padded_dense, segment_reduce  # noqa: E402

# the kernels' constants (a changed one fails test_the_shapes_cross_the_thresholds_they_are_meant_for, not silently the coverage)
JG_THREADS = 256  # csrc/jagged_ops.hip:11
JG_GRID = 16384   # csrc/jagged_ops.hip:62, :81, :137, :154 grid cap of the grid-stride kernels

TAIL_SHAPE = (37, 64, 5, 200)      # B, D, max_len, longest sequence
GRID_SHAPE = (4_100, 64, 64, 70)
SEGMENT_SHAPES = [(300, 36, 300), (65_600, 256, 2)]  # S, D, longest segment
SEGMENT_STRIDED = (40, 256, 50)
PAD_COLS, COL0 = 12, 4  # rows live in columns [4, 4 + D) of buffers 12 floats wider
U = 2.0 ** -24  # fp32 unit roundoff


def test_the_shapes_cross_the_thresholds_they_are_meant_for():
    B, D, max_len, longest = TAIL_SHAPE
    assert (longest - max_len) * (D // 4) > 4 * JG_THREADS  # tzr_jagged_zero_tail_kernel: several passes of its workgroup's loop
    B, D, max_len, longest = GRID_SHAPE
    assert 4_100 * 64 * 16 > JG_GRID * JG_THREADS and B * max_len * (D // 4) > JG_GRID * JG_THREADS and longest > max_len
    (s0, d0, l0), (s1, d1, l1) = SEGMENT_SHAPES
    assert l0 >= 300 and d0 % 8 == 4 and s0 * (d0 // 4) > JG_THREADS  # hundreds of rows, an odd count of float4, several workgroups
    assert s1 * (d1 // 4) > JG_GRID * JG_THREADS
    assert PAD_COLS % 4 == 0 and COL0 % 4 == 0 and 0 < COL0 < PAD_COLS  # 16-byte aligned rows with padding on both sides


def _offsets(lens):
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lens, 0)
    return off


def _jagged_case(seed, B, D, max_len, longest):
    """lengths with empty, exactly-full, one-short, one-over and the longest sequence among them; values; the oracle's dense form
    and the jagged gradient of a random dense gradient"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest + 1, size=B).astype(np.int64)
    lens[:6] = [0, max_len, max(max_len - 1, 0), max_len + 1, longest, 0]
    lens = torch.from_numpy(lens)
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(int(lens.sum()), D, generator=g)
    go = torch.randn(B, max_len, D, generator=g)
    vr = v.clone().requires_grad_(True)
    ref = orc.jagged_to_padded_dense(vr, lens, max_len, -1.5)
    ref.backward(go)
    return lens, _offsets(lens), v, go, ref.detach(), vr.grad


def _truncated_rows(lens, max_len):
    off = _offsets(lens)
    return torch.cat([torch.arange(int(off[b]) + max_len, int(off[b + 1])) for b in range(len(lens)) if lens[b] > max_len])


def _run_jagged_wrapper(dev, off, v, go, max_len):
    vd = v.clone().to(dev).requires_grad_(True)
    out = jagged_to_padded_dense(vd, off.to(dev), max_len, -1.5)
    out.backward(go.to(dev))
    return out.detach().cpu(), vd.grad.cpu()


def test_jagged_dense_with_long_truncated_tails(dev):
    B, D, max_len, longest = TAIL_SHAPE
    lens, off, v, go, ref, ref_grad = _jagged_case(1, B, D, max_len, longest)
    out, grad = _run_jagged_wrapper(dev, off, v, go, max_len)
    assert torch.equal(out, ref)  # a copy: bit-exact
    assert torch.equal(grad, ref_grad)
    cut = _truncated_rows(lens, max_len)
    assert len(cut) > B * (longest - max_len) // 4 and not grad[cut].any()  # truncated positions: exactly zero


def test_jagged_dense_on_column_slices_of_wider_buffers(dev):
    """`values_stride > dim` through the C entries (the wrapper makes contiguous copies): the forward reads, and the backward
    writes, rows that are column slices of NaN-filled buffers; the padding columns stay NaN, truncated rows become zero."""
    B, D, max_len, longest = TAIL_SHAPE
    lens, off, v, go, ref, ref_grad = _jagged_case(2, B, D, max_len, longest)
    N, wide = v.shape[0], D + PAD_COLS
    L = _lib.lib()
    d_off = off.to(dev)
    vbuf = torch.full((N, wide), float("nan"))
    vbuf[:, COL0:COL0 + D] = v
    vbuf = vbuf.to(dev)
    vs = vbuf[:, COL0:COL0 + D]
    out = torch.full((B, max_len, D), float("nan"), device=dev)
    _lib.check(L.tzr_jagged_to_padded_dense(_lib.ptr(vs), vs.stride(0), _lib.ptr(d_off), B, max_len, D, -1.5, _lib.ptr(out),
                                            _lib.stream_ptr(dev)), "tzr_jagged_to_padded_dense")
    assert vs.stride(0) == wide and torch.equal(out.cpu(), ref)
    gbuf = torch.full((N, wide), float("nan"), device=dev)
    gs = gbuf[:, COL0:COL0 + D]
    d_go = go.to(dev)
    _lib.check(L.tzr_padded_dense_to_jagged(_lib.ptr(d_go), _lib.ptr(d_off), B, max_len, D, _lib.ptr(gs), gs.stride(0),
                                            _lib.stream_ptr(dev)), "tzr_padded_dense_to_jagged")
    gbuf = gbuf.cpu()
    assert torch.equal(gbuf[:, COL0:COL0 + D], ref_grad)  # every row written: the gradient, or zero behind max_len
    assert not gbuf[_truncated_rows(lens, max_len), COL0:COL0 + D].any()
    assert gbuf[:, :COL0].isnan().all() and gbuf[:, COL0 + D:].isnan().all()
    assert torch.equal(vbuf.cpu()[:, COL0:COL0 + D], v)  # the input is only read


def test_jagged_dense_with_max_len_zero(dev):
    """every sequence is truncated to nothing: the forward writes nothing, the backward zeroes every row"""
    B, D = 9, 8
    lens = torch.tensor([3, 0, 1, 300, 0, 2, 7, 1, 4])
    off, N = _offsets(lens), int(lens.sum())
    v = torch.randn(N, D)
    out, grad = _run_jagged_wrapper(dev, off, v, torch.zeros(B, 0, D), 0)
    assert tuple(out.shape) == (B, 0, D) and tuple(grad.shape) == (N, D) and not grad.any()
    L = _lib.lib()
    d_off, d_v = off.to(dev), v.to(dev)
    dense = torch.full((16,), -7.0, device=dev)
    _lib.check(L.tzr_jagged_to_padded_dense(_lib.ptr(d_v), D, _lib.ptr(d_off), B, 0, D, -1.5, _lib.ptr(dense), _lib.stream_ptr(dev)),
               "tzr_jagged_to_padded_dense")
    gbuf = torch.full((N, D + PAD_COLS), float("nan"), device=dev)
    gs = gbuf[:, COL0:COL0 + D]
    _lib.check(L.tzr_padded_dense_to_jagged(_lib.ptr(dense), _lib.ptr(d_off), B, 0, D, _lib.ptr(gs), gs.stride(0), _lib.stream_ptr(dev)),
               "tzr_padded_dense_to_jagged")
    gbuf = gbuf.cpu()
    assert (dense.cpu() == -7.0).all()
    assert not gbuf[:, COL0:COL0 + D].any() and gbuf[:, :COL0].isnan().all() and gbuf[:, COL0 + D:].isnan().all()


def test_jagged_dense_past_the_grid_cap(dev):
    """more float4 than 16 384 workgroups of 256 lanes cover at once: the grid-stride second pass, forward and backward"""
    B, D, max_len, longest = GRID_SHAPE
    lens, off, v, go, ref, ref_grad = _jagged_case(3, B, D, max_len, longest)
    out, grad = _run_jagged_wrapper(dev, off, v, go, max_len)
    assert torch.equal(out, ref)
    assert torch.equal(grad, ref_grad)


# ---- segment reduce -----------------------------------------------------------------------------------------------------

def _segment_case(seed, S, D, longest):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest + 1, size=S).astype(np.int64)
    lens[rng.integers(0, S, size=max(3, S // 20))] = 0  # empty segments
    lens[[0, S // 2, S - 1]] = [longest, 1, longest]
    lens = torch.from_numpy(lens)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(int(lens.sum()), D, generator=g)
    go = torch.randn(S, D, generator=g)
    return lens, x, go


def _segment_reference(lens, x, go, pooling):
    """float64 torch.segment_reduce + nan_to_num and its autograd; the error bounds of the kernel's arithmetic (a segment's rows
    added in order in fp32, then one product with the fp32 reciprocal of the length), evaluated in float64 from the inputs:
    forward (len + 2) u sum|x_i| per output element (the sum's (len - 1) u, the reciprocal's and the product's u each, one u
    for the second-order terms; a mean divides it by len), backward 3 u |ref| (reciprocal and product)."""
    xr = x.double().requires_grad_(True)
    ref = torch.nan_to_num(torch.segment_reduce(xr, pooling, lengths=lens), nan=0.0)
    ref.backward(go.double())
    sum_abs = torch.segment_reduce(x.double().abs(), "sum", lengths=lens)
    n = lens.double()[:, None]
    fwd_bound = (n + 2) * U * sum_abs / (n.clamp(min=1) if pooling == "mean" else 1.0)
    return ref.detach(), fwd_bound, xr.grad, 3 * U * xr.grad.abs()


def _assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    ratio = (err / bound)[bound > 0]
    print(f"{what}: max err {err.max().item():.3e}, largest err / bound {ratio.max().item() if ratio.numel() else 0.0:.3f}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("S,D,longest", SEGMENT_SHAPES)
def test_segment_reduce_long_segments_and_past_the_grid_cap(dev, S, D, longest, pooling):
    lens, x, go = _segment_case(S, S, D, longest)
    ref, fwd_bound, ref_grad, bwd_bound = _segment_reference(lens, x, go, pooling)
    xd = x.clone().to(dev).requires_grad_(True)
    out = segment_reduce(xd, lens.to(dev), pooling)
    out.backward(go.to(dev))
    _assert_within(out.detach().cpu(), ref, fwd_bound, f"forward {pooling} S={S}")
    _assert_within(xd.grad.cpu(), ref_grad, bwd_bound, f"backward {pooling} S={S}")
    assert not out.detach().cpu()[lens == 0].any()  # an empty segment: a zero row, not NaN
    out2 = segment_reduce(x.to(dev), lens.to(dev), pooling)
    assert torch.equal(out2, out.detach())  # deterministic


@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_segment_reduce_on_column_slices_of_wider_buffers(dev, pooling):
    """`values` and `seg` strided in both directions through the C entries, as the call of the DIN tower's backward passes them
    (sequence.py: a column block of the hidden gradient reduced per sample): NaN around the slices stays NaN."""
    S, D, longest = SEGMENT_STRIDED
    lens, x, go = _segment_case(5, S, D, longest)
    ref, fwd_bound, ref_grad, bwd_bound = _segment_reference(lens, x, go, pooling)
    N, wide, mode = x.shape[0], D + PAD_COLS, int(pooling == "mean")
    L = _lib.lib()
    d_off = _offsets(lens).to(dev)

    def framed(rows, inner=None):
        buf = torch.full((rows, wide), float("nan"))
        if inner is not None:
            buf[:, COL0:COL0 + D] = inner
        buf = buf.to(dev)
        return buf, buf[:, COL0:COL0 + D]

    xbuf, xs = framed(N, x)
    obuf, os_ = framed(S)
    _lib.check(L.tzr_segment_reduce_fwd(_lib.ptr(xs), xs.stride(0), _lib.ptr(d_off), S, D, mode, _lib.ptr(os_), os_.stride(0),
                                        _lib.stream_ptr(dev)), "tzr_segment_reduce_fwd")
    obuf = obuf.cpu()
    _assert_within(obuf[:, COL0:COL0 + D], ref, fwd_bound, f"strided forward {pooling}")
    assert obuf[:, :COL0].isnan().all() and obuf[:, COL0 + D:].isnan().all()
    assert torch.equal(obuf[:, COL0:COL0 + D], segment_reduce(x.to(dev), lens.to(dev), pooling).cpu())  # same order, same bits
    gbuf, gs = framed(S, go)
    vbuf, vs = framed(N)
    _lib.check(L.tzr_segment_reduce_bwd(_lib.ptr(gs), gs.stride(0), _lib.ptr(d_off), S, D, mode, _lib.ptr(vs), vs.stride(0),
                                        _lib.stream_ptr(dev)), "tzr_segment_reduce_bwd")
    vbuf = vbuf.cpu()
    _assert_within(vbuf[:, COL0:COL0 + D], ref_grad, bwd_bound, f"strided backward {pooling}")
    assert vbuf[:, :COL0].isnan().all() and vbuf[:, COL0 + D:].isnan().all()
    assert torch.equal(xbuf.cpu()[:, COL0:COL0 + D], x) and torch.equal(gbuf.cpu()[:, COL0:COL0 + D], go)  # inputs are only read
