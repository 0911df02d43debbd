"""The QUint8RowwiseF16 row format in numpy, written from its description in include/tzrec_hip.h (tzr_quantize_rows_q8f16,
tzr_dequantize_rows_q8f16): a row of `dim` float values becomes [dim uint8 values][float16 scale][float16 offset], dim + 4 bytes,
little-endian.  tests/test_export_widths.py first shows that this reproduces the reference encoder's recorded outputs byte for
byte (tests/golden/reference_quant_vectors.npz), then holds the kernels to it at widths the recording does not have.
Nothing here touches the package under test.

Every step is one IEEE single-precision operation: per-row min and max; offset = fp16(min); scale = fp16((max - offset) / 255),
1 where the range is 0 or the fp16 scale is 0; q = rint((x - offset) / scale) clipped to 0..255.  Decoding: q * scale + offset,
the product rounded before the sum."""
import numpy as np

INT64_MAX = (1 << 63) - 1
FP16_MAX = 65504.0


def encode(x):
    """float32 (or float16, widened first) [rows, dim] -> uint8 [rows, dim + 4]"""
    x = np.ascontiguousarray(x).astype(np.float32)
    rows = x.shape[0]
    off16 = x.min(axis=1).astype(np.float16)
    off = off16.astype(np.float32)
    span = x.max(axis=1) - off
    with np.errstate(divide="ignore", invalid="ignore"):
        scale16 = np.where(span != 0, span / np.float32(255.0), np.float32(1.0)).astype(np.float32).astype(np.float16)
        scale16 = np.where(scale16 == 0, np.float16(1.0), scale16).astype(np.float16)
        scale = scale16.astype(np.float32)
        q = np.clip(np.rint((x - off[:, None]) / scale[:, None]), 0.0, 255.0).astype(np.uint8)
    meta = np.stack([scale16, off16], axis=1).astype("<f2").view(np.uint8).reshape(rows, 4)
    return np.concatenate([q, meta], axis=1)


def decode(rows, dim):
    """uint8 [rows, dim + 4] -> float32 [rows, dim]"""
    rows = np.ascontiguousarray(rows)
    assert rows.dtype == np.uint8 and rows.shape[1] == dim + 4
    meta = rows[:, dim:].copy().view("<f2").astype(np.float32)
    prod = rows[:, :dim].astype(np.float32) * meta[:, :1]
    return (prod + meta[:, 1:2]).astype(np.float32)


def first_bad(x):
    """[3] the smallest row index with a non-finite value / an offset / a scale outside the finite float16 range -- one kind per
    row, a non-finite value before the offset before the scale -- INT64_MAX where there is none"""
    x = np.asarray(x, dtype=np.float32)
    out = [INT64_MAX] * 3
    for r in range(x.shape[0] - 1, -1, -1):
        row = x[r]
        if not np.isfinite(row).all():
            out[0] = r
            continue
        if abs(float(row.min())) > FP16_MAX:
            out[1] = r
        elif abs(float(row.max()) - float(row.min().astype(np.float16))) > FP16_MAX * 255.0:
            out[2] = r
    return out
