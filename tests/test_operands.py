"""_lib.rows_ok / _lib.rows16: the Python mirror of tzr_rows_operand (csrc/tzr_common.h), the one rule for a [B, H] float4 row
operand -- fp32, 2-D, unit column stride, row stride a multiple of 4 floats and at least the width, 16-byte aligned data.  One
table of tensors against both; no library is loaded."""
import pytest
import torch

from torcheasyrec_amd import _lib


def _base(rows, cols):
    """a [rows, cols] fp32 tensor at a 16-byte aligned address (so that every offset below is what it says)"""
    t = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols)
    assert t.data_ptr() % 16 == 0
    return t


# name -> (the tensor, taken as it is)
TABLE = {
    "contiguous": (lambda: _base(3, 8), True),
    "column_slice": (lambda: _base(3, 16)[:, 4:12], True),
    "misaligned": (lambda: _base(3, 16)[:, 1:9], False),
    "row_stride_10": (lambda: _base(3, 10)[:, :8], False),
    "expanded": (lambda: _base(1, 8).expand(3, 8), False),
    "transposed": (lambda: _base(8, 3).t(), False),
    "one_row_of_stride_10": (lambda: _base(4, 10)[1:2, :8], False),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_rows_ok_and_rows16(name):
    make, taken = TABLE[name]
    t = make()
    assert _lib.rows_ok(t) is taken
    assert _lib.rows_ok(t, t.shape[1]) is taken and not _lib.rows_ok(t, t.shape[1] + 4)
    r = _lib.rows16(t)
    if taken:
        assert r is t and r.data_ptr() == t.data_ptr()
    else:
        assert r.data_ptr() != t.data_ptr() and _lib.rows_ok(r, t.shape[1]) and torch.equal(r, t)
        assert r.stride() == (t.shape[1], 1)  # (the one-row slice too: .contiguous() would return it unchanged)


def test_one_row_slice_is_what_contiguous_keeps():
    """why rows16 clones: .contiguous() calls a one-row tensor contiguous whatever its row stride and address"""
    t = _base(4, 10)[1:2, :8]
    assert t.contiguous().data_ptr() == t.data_ptr() and t.data_ptr() % 16 == 8 and t.stride(0) == 10


@pytest.mark.parametrize("make", [lambda: _base(3, 8).double(), lambda: _base(3, 8).half(), lambda: _base(1, 8)[0]],
                         ids=["fp64", "fp16", "one_dim"])
def test_rows_ok_refuses_outright(make):
    assert not _lib.rows_ok(make())


def test_scalar_rows_is_the_weaker_rule():
    """the kernels that read rows float by float take misaligned rows and any row stride that keeps rows apart"""
    for name in ("misaligned", "row_stride_10", "one_row_of_stride_10"):
        t = TABLE[name][0]()
        assert _lib.scalar_rows(t) is t and _lib.scalar_row_stride(t) >= t.shape[1]
    for name in ("expanded", "transposed"):
        t = TABLE[name][0]()
        r = _lib.scalar_rows(t)
        assert r is not t and r.is_contiguous()


def test_rows3_ok():
    """[B, K, D]: the B K rows of one row operand, one stride between all of them"""
    wide = _base(6, 16)
    assert _lib.rows3_ok(_base(6, 8).view(3, 2, 8)) and _lib.rows3_ok(wide[:, 4:12].view(3, 2, 8))
    assert not _lib.rows3_ok(wide[:, 1:9].view(3, 2, 8)) and not _lib.rows3_ok(_base(6, 10)[:, :8].view(3, 2, 8))
    assert not _lib.rows3_ok(_base(6, 8).view(2, 3, 8).transpose(0, 1)) and not _lib.rows3_ok(_base(6, 8).view(3, 2, 8).double())
