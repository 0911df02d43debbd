"""The INT8 row-wise export (csrc/export_ops.hip: tzr_quantize_rows_q8f16, tzr_dequantize_rows_q8f16) at every lane-group class
of its mapping -- lg = dim / 4 lanes per row, gpw = 64 // lg rows per wave and slot: power-of-two groups (shuffle trees),
other groups (the lane-by-lane reductions), groups that leave idle tail lanes in a wave (64 % lg != 0), dim > 128 -- with three
workgroups each, the last one partial, byte for byte against the numpy restatement of the format (tests/quant_ref.py), which the
first test ties to the reference encoder's recorded outputs."""
import os

import numpy as np
import pytest
import torch

import quant_ref
from torcheasyrec_amd import _lib

_Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_quant_vectors.npz"))
DIMS = [4, 8, 12, 20, 24, 28, 32, 36, 48, 64, 96, 100, 128, 192, 252, 256]
EX_WAVES, EX_U, WAVE = 4, 4, 64  # export_ops.hip:16,18: waves of a workgroup, row slots of a wave and iteration
GUARD = 0xAB


def n_rows(dim):
    """two full workgroups, one full row slot of the third's first wave and one row of the next slot"""
    gpw = WAVE // (dim // 4)
    return 2 * EX_WAVES * EX_U * gpw + gpw + 1


def test_the_restatement_is_the_reference_encoder():
    """byte for byte at the five recorded widths: q_D from x_D, dq_D from q_D"""
    for D in (4, 12, 16, 64, 128):
        np.testing.assert_array_equal(quant_ref.encode(_Z[f"x_{D}"]), _Z[f"q_{D}"])
        got = quant_ref.decode(_Z[f"q_{D}"], D)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), _Z[f"dq_{D}"].view(np.uint32))


def test_the_widths_reach_every_lane_group_class():
    lgs = [d // 4 for d in DIMS]
    assert all(d % 4 == 0 and d <= 256 for d in DIMS) and max(DIMS) == 256 and sum(d > 128 for d in DIMS) >= 3
    assert {lg for lg in lgs if lg & (lg - 1) == 0} == {1, 2, 8, 16, 32, 64}  # the shuffle trees (lg = 4 is dim 16 of tests/test_export_quant.py)
    odd = [lg for lg in lgs if lg & (lg - 1)]
    assert len(odd) >= 8 and all(WAVE % lg != 0 for lg in odd)  # (64 has no other divisors: each of them leaves idle tail lanes)
    assert {WAVE // lg for lg in odd} >= {1, 2, 5, 7, 9, 10, 12, 21}  # rows per wave next to idle tail lanes
    for d in DIMS:
        gpw = WAVE // (d // 4)
        wg = EX_WAVES * EX_U * gpw
        assert -(-n_rows(d) // wg) == 3 and n_rows(d) - 2 * wg == gpw + 1


def table(dim, seed):
    """randn rows times a per-row scale in (0, 10); a constant row, an all-zero row, a row of equal values but the first, rows
    holding +-65504 -- at the head of the table and in its last, partial workgroup"""
    rows = n_rows(dim)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=g) * (torch.rand(rows, 1, generator=g) * 9.99 + 0.005)
    for base in (1, rows - 7):
        x[base] = 3.25
        x[base + 1] = 0.0
        x[base + 2] = -1.5
        x[base + 2, 0] = 2.0
        x[base + 3, 0] = 65504.0
        x[base + 4, dim - 1] = -65504.0
        x[base + 5, 0], x[base + 5, dim - 1] = 65504.0, -65504.0
    return x


def quantize(dev, view, dim):
    """the entry point on a 2-D view of unit column stride -> (uint8 [rows, dim + 4] as numpy, first_bad [3])"""
    rows = view.shape[0]
    out = torch.full((rows * (dim + 4) + 4,), GUARD, dtype=torch.uint8, device=dev)
    bad = torch.zeros(3, dtype=torch.int64, device=dev)
    dt = _lib.DT_F16 if view.dtype == torch.float16 else _lib.DT_F32
    assert view.stride(1) == 1 and view.data_ptr() % 16 == 0
    assert _lib.lib().tzr_quantize_rows_q8f16(_lib.ptr(view), dt, view.stride(0), rows, dim, _lib.ptr(out), _lib.ptr(bad), _lib.stream_ptr(dev)) == 0
    got = out.cpu().numpy()
    assert (got[rows * (dim + 4):] == GUARD).all()  # nothing behind the last row was written
    return got[:rows * (dim + 4)].reshape(rows, dim + 4), bad.cpu().tolist()


def dequantize(dev, q, dim):
    """the entry point with out_stride = dim + 8, into a NaN-filled tensor -> float32 [rows, dim] as numpy"""
    rows = q.shape[0]
    wide = torch.full((rows, dim + 8), float("nan"), dtype=torch.float32, device=dev)
    v = wide[:, 4:4 + dim]
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    assert _lib.lib().tzr_dequantize_rows_q8f16(_lib.ptr(qd), rows, dim, _lib.ptr(v), wide.stride(0), _lib.stream_ptr(dev)) == 0
    assert bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 4 + dim:]).all())
    return v.cpu().numpy().copy()


@pytest.mark.parametrize("dim", DIMS)
def test_every_width_is_byte_equal(dev, dim):
    x = table(dim, seed=dim)
    want = quant_ref.encode(x.numpy())
    clean = [quant_ref.INT64_MAX] * 3
    got, bad = quantize(dev, x.to(dev), dim)
    np.testing.assert_array_equal(got, want)
    assert bad == clean
    wide = torch.full((x.shape[0], 2 * dim), float("nan"), device=dev)  # the left half of an interleaved [w | m] allocation
    wide[:, :dim] = x.to(dev)
    got, bad = quantize(dev, wide[:, :dim], dim)
    np.testing.assert_array_equal(got, want)
    assert bad == clean
    half = x.to(torch.float16)
    got, bad = quantize(dev, half.to(dev), dim)
    np.testing.assert_array_equal(got, quant_ref.encode(half.float().numpy()))  # the fp16 values widened to fp32
    assert bad == clean
    back = dequantize(dev, want, dim)
    np.testing.assert_array_equal(back.view(np.uint32), quant_ref.decode(want, dim).view(np.uint32))


def test_first_bad_holds_the_smallest_row_of_each_kind(dev):
    """dim = 20: 12 rows per wave and slot, 192 per workgroup.  A row reports one kind (a non-finite value before the offset
    before the scale), so the three firsts are different rows -- one per workgroup here, each with a later second"""
    dim, rows = 20, 700
    x = torch.randn(rows, dim, generator=torch.Generator().manual_seed(20))
    nan_rows, offset_rows, scale_rows = (3, 400), (200, 250, 500), (390, 600)
    for r in nan_rows:
        x[r, 7] = float("nan")
    x[3, :4] = 70000.0  # its minimum (NaN aside) is out of range too: still a row of the first kind only
    x[400, 2] = float("inf")
    for r in offset_rows:
        x[r] = 70000.0 + torch.arange(dim) / 4.0
    x[250, 0], x[250, 1] = -70000.0, 3.0e7  # offset and scale out of range: a row of the second kind only
    for r in scale_rows:
        x[r, 0], x[r, dim - 1] = -65504.0, 2.0e7
    assert [r // 192 for r in (nan_rows[0], offset_rows[0], scale_rows[0])] == [0, 1, 2]
    assert quant_ref.first_bad(x.numpy()) == [3, 200, 390]
    got, bad = quantize(dev, x.to(dev), dim)
    assert bad == [3, 200, 390]
    good = np.ones(rows, bool)
    good[list(nan_rows + offset_rows + scale_rows)] = False
    ok = x.clone()
    ok[~torch.from_numpy(good)] = 0.0
    np.testing.assert_array_equal(got[good], quant_ref.encode(ok.numpy())[good])  # the rows around them are encoded as ever
    got, bad = quantize(dev, ok.to(dev), dim)
    assert bad == [quant_ref.INT64_MAX] * 3
    np.testing.assert_array_equal(got, quant_ref.encode(ok.numpy()))
