"""tzr_lookup_grads (csrc/sharded_ops.hip), the requester-side backward of the id-granularity sharded exchange, called through
the C entry point against its float64 restatement (tests/lookup_grads_ref.py): one gradient row per exchanged id.

Every group gradient is a column slice (from column 4) of a wider tensor that is NaN outside the slice; the output is
[N + extra, D + pad] filled with a sentinel that rows nobody addresses and columns >= D must keep bit for bit.

Bound, per element: |got - want| <= (n_dst + 2) 2^-24 (sum_groups |grad_g|) |scale| -- the kernel's n_dst - 1 additions, the
reciprocal, w * inv and the product per component are each rounded once to fp32; `want` and the magnitudes are float64 on the
fp32 inputs.  Largest observed / bound over the cases below (printed per case):
  lane emulator: 0.07 - 0.71 with per-id weights; 0.24 - 0.50 without, ragged; 0.00 - 0.44 without, uniform (0.00: every lookup of
                 the case reads one group, so its rows are copies)
  MI355X:        the same figure as the emulator's in each of the 176 cases
Sum pooling without weights over one group, and the dyadic case (gradients k/64, weights in {0.5, 1, 2}, bags of 1, 2 or 4
ids), are exact: compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import lookup_grads_ref as ref
from torcheasyrec_amd import _lib
from torcheasyrec_amd.ops import grad_dsts

# the kernel's constants, read from its source: a changed one fails test_the_shapes_cross_the_branches_they_are_meant_for, not
# silently the coverage
_SRC = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "sharded_ops.hip")).read()
SH_THREADS = int(re.search(r"#define SH_THREADS (\d+)", _SRC).group(1))
SH_MAXKEYS = int(re.search(r"#define SH_MAXKEYS (\d+)", _SRC).group(1))
TILE_SWITCH_B, TILE_SMALL, TILE_LARGE = map(int, re.search(r"tile_b = B <= (\d+) \? (\d+) : (\d+);", _SRC).groups())

# (B, lookups F, D, groups)
RAGGED_SHAPES = [(1, 1, 4, 1),
                 (7, 3, 16, 2), (8, 3, 16, 2), (9, 3, 16, 2), (17, 3, 16, 2),
                 (3, 256, 4, 8), (3, 257, 4, 8), (2, 513, 8, 5),
                 (5, 7, 36, 3), (5, 7, 128, 3), (2, 3, 256, 2)]
LARGE_SHAPES = [(16384, 1, 4, 1), (16385, 1, 4, 1)]  # uniform, no weights
# (weighted, permuted, extra, pad)
MODES = [(w, p, 5 if p else 0, pad) for w in (False, True) for p in (False, True) for pad in (0, 4)]
EXTRA = 5
SENTINEL_BITS = int(np.float32(ref.SENTINEL).view(np.int32))


def test_the_shapes_cross_the_branches_they_are_meant_for():
    assert (SH_THREADS, SH_MAXKEYS, TILE_SWITCH_B, TILE_SMALL, TILE_LARGE) == (256, 256, 16384, 8, 32)
    bs = [s[0] for s in RAGGED_SHAPES[1:5]]
    assert bs == [TILE_SMALL - 1, TILE_SMALL, TILE_SMALL + 1, 2 * TILE_SMALL + 1]  # one short, exact, one over, two tiles and one
    fs = [s[1] for s in RAGGED_SHAPES[5:8]]
    assert fs == [SH_MAXKEYS, SH_MAXKEYS + 1, 2 * SH_MAXKEYS + 1]  # one LDS pass exactly, one lookup into the second, three passes
    assert RAGGED_SHAPES[5][3] == RAGGED_SHAPES[6][3] == _lib.TZR_MAX_DST
    lgs = [s[2] // 4 for s in RAGGED_SHAPES[8:]]
    assert lgs == [9, 32, 64] and lgs[0] & (lgs[0] - 1) and 4 * lgs[2] == 256  # not a power of two; the widest a table can be
    assert all(s[0] <= TILE_SWITCH_B for s in RAGGED_SHAPES)
    (b0, *_), (b1, *_) = LARGE_SHAPES
    assert b0 == TILE_SWITCH_B and b1 == TILE_SWITCH_B + 1 and b1 % TILE_LARGE == 1  # last B on the small tile; first on the large
    # one workgroup's items fit an int: the kernel counts them in one
    assert TILE_LARGE * SH_MAXKEYS * 64 < 2 ** 31
    # what the draws are meant to contain, they contain
    seen_n, seen_pool = set(), set()
    for shape in RAGGED_SHAPES:
        c = ref.draw(*shape, ragged=True)
        seen_n |= set(c.n_dst.tolist())
        seen_pool |= set(c.pool.tolist())
        assert c.n_dst.max() <= min(4, shape[3]) and sorted(c.key.tolist()) == list(range(shape[1]))
        assert all(len(set(c.dst[f, :c.n_dst[f]].tolist())) == c.n_dst[f] for f in range(shape[1]))  # distinct groups
        if shape[1] > 1:
            assert not np.array_equal(c.key, np.arange(shape[1]))  # not the identity
            assert len(set(c.col[:, 0].tolist())) > 1  # lookups read different offsets
        if shape[0] * shape[1] >= 2:
            lens = c.lens.reshape(shape[1], shape[0])[c.key]  # [lookup, sample]
            assert (lens == 0).any() and (lens[c.pool == 1] == 1).any() and (lens[c.pool == 1] > 1).any()
            assert c.lens.max() <= 4
    assert seen_n == {1, 2, 3, 4} and seen_pool == {0, 1}


def _wide(g, dev):
    """`g` [B, w] as a column slice, from column 4, of a wider tensor that is NaN elsewhere; row stride w + 8"""
    B, w = g.shape
    t = torch.full((B, w + 8), float("nan"), dtype=torch.float32, device=dev)
    v = t[:, 4:4 + w]
    v.copy_(torch.tensor(g))
    assert v.stride(0) % 4 == 0 and v.stride(0) > w and v.data_ptr() % 16 == 0 and v.data_ptr() != t.data_ptr()
    return t, v


def _feats(c):
    feats = np.zeros(c.F, dtype=_lib.FEATURE_DT)
    feats["key"], feats["n_dst"], feats["dst"], feats["col"] = c.key, c.n_dst, c.dst, c.col
    feats["pooling"] = np.where(c.pool == 1, _lib.POOL_MEAN, _lib.POOL_SUM)
    feats["order"] = np.arange(c.F)
    return feats


def _run(dev, c):
    """the library's output for case `c`, as a numpy array"""
    # (every device tensor is named until after the sync: a temporary's block would go back to the caching allocator -- and to
    # the next upload -- before the launch, tests/test_index_parity.py::test_rows_gather_matches_indexing)
    wides, views = zip(*[_wide(g, dev) for g in c.grads])
    d_feats = _lib.upload_struct(_feats(c), dev)
    d_off = torch.tensor(c.offsets).to(dev) if c.ragged else None
    d_w = torch.tensor(c.weights).to(dev) if c.weights is not None else None
    d_pos = torch.tensor(c.positions).to(dev) if c.positions is not None else None
    out = torch.full((c.rows, c.D + c.pad), float(ref.SENTINEL), dtype=torch.float32, device=dev)
    gd = grad_dsts(views)
    rc = _lib.lib().tzr_lookup_grads(_lib.ptr(d_feats), c.F, _lib.ptr(d_off), _lib.ptr(d_w), c.B, 0 if c.ragged else 1, _lib.ptr(d_pos),
                                     gd, len(views), _lib.ptr(out), c.D + c.pad, c.D, _lib.stream_ptr(dev))
    _lib.check(rc, "tzr_lookup_grads")
    if dev.type == "cuda":
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    del wides, views, d_feats, d_off, d_w, d_pos, gd
    return got


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(c, got, what, exact=False):
    assert got.shape == c.want.shape
    assert not np.isnan(got).any(), f"{what}: NaN from outside a gradient slice reached the output"
    # rows no position addresses, and columns >= D, hold the sentinel bit for bit
    keep = np.ones(got.shape, dtype=bool)
    keep[c.written, :c.D] = False
    assert np.array_equal(_bits(got)[keep], np.full(int(keep.sum()), SENTINEL_BITS, dtype=np.int32)), f"{what}: sentinel overwritten"
    assert c.written.sum() == c.N
    g, w, bd = got[c.written, :c.D].astype(np.float64), c.want[c.written, :c.D], c.bound[c.written, :c.D]
    err = np.abs(g - w)
    ratio = float(np.max(err / np.where(bd > 0, bd, 1.0), initial=0.0))
    print(f"lookup_grads {what}: largest |got - want| / bound = {ratio:.3f}")
    assert (err <= bd).all(), f"{what}: largest |got - want| / bound = {ratio:.3f}"
    if exact:
        assert np.array_equal(g, w) and np.array_equal(_bits(g), _bits(w)), f"{what}: not bit-equal to the float64 result"


@pytest.mark.parametrize("weighted,permuted,extra,pad", MODES)
@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "uniform"])
def test_matches_float64(dev, ragged, shape, weighted, permuted, extra, pad):
    c = ref.draw(*shape, ragged=ragged, weighted=weighted, permuted=permuted, extra=extra, pad=pad)
    assert c.rows == max(c.N + extra, 1) and (ragged or c.N == shape[0] * shape[1])
    _check(c, _run(dev, c), f"{shape} {'ragged' if ragged else 'uniform'} w={weighted} pos={permuted} pad={pad} on {dev.type}")


@pytest.mark.parametrize("shape", LARGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sample_tile_switch(dev, shape):
    """B = 16384 is the last batch on the sample tile of 8, 16385 the first on 32 (with a one-sample tail tile); one-id bags with
    mean pooling: the identity, bit for bit"""
    c = ref.draw(*shape, ragged=False, pooling=1)
    got = _run(dev, c)
    _check(c, got, f"{shape} uniform on {dev.type}", exact=True)
    assert np.array_equal(_bits(got), _bits(c.grads[0]))  # D = 4, one lookup, one group: the output IS the gradient


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "uniform"])
@pytest.mark.parametrize("shape", [(9, 3, 16, 2), (3, 257, 4, 8), (5, 7, 36, 3)], ids=lambda s: "x".join(map(str, s)))
def test_sum_of_one_group_is_a_copy(dev, shape, ragged):
    """sum pooling, no weights, one group: every output row equals its gradient slice bit for bit (uniform: also under mean
    pooling, the mean of a one-id bag)"""
    for pooling in ([0] if ragged else [0, 1]):
        c = ref.draw(*shape, ragged=ragged, permuted=True, extra=EXTRA, pad=4, n_dst=(1, 1), pooling=pooling)
        _check(c, _run(dev, c), f"{shape} copy pooling={pooling} on {dev.type}", exact=True)


@pytest.mark.parametrize("shape", [(9, 3, 16, 4), (3, 257, 4, 8), (5, 7, 36, 4)], ids=lambda s: "x".join(map(str, s)))
def test_dyadic_case_is_exact(dev, shape):
    """gradients k/64, weights in {0.5, 1, 2}, bags of 1, 2 or 4 ids, mean pooling over 2 to 4 groups: no operation rounds, so the
    output equals the float64 result bit for bit"""
    c = ref.draw(*shape, ragged=True, weighted=True, permuted=True, extra=EXTRA, pad=4, n_dst=(2, 4), pooling=1, dyadic=True)
    assert set(c.lens.tolist()) == {1, 2, 4} and set(c.n_dst.tolist()) <= {2, 3, 4} and set(c.weights.tolist()) == {0.5, 1.0, 2.0}
    assert shape[1] < 100 or set(c.n_dst.tolist()) == {2, 3, 4}
    assert float(c.bound.max()) > 0 and np.array_equal(c.want, c.want.astype(np.float32))
    _check(c, _run(dev, c), f"{shape} dyadic on {dev.type}", exact=True)


@pytest.mark.parametrize("shape", [(17, 3, 16, 2), (3, 257, 4, 8), (5, 7, 36, 3)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bit_equal(dev, shape):
    c = ref.draw(*shape, ragged=True, weighted=True, permuted=True, extra=EXTRA, pad=4)
    assert np.array_equal(_bits(_run(dev, c)), _bits(_run(dev, c)))


def test_abi(dev):
    """what the entry point refuses with TZR_ERR_INVALID before it launches anything; B = 0 is TZR_OK and writes nothing"""
    c = ref.draw(9, 3, 16, 2, ragged=True, weighted=True, permuted=True, extra=EXTRA, pad=4)
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    wides, views = zip(*[_wide(g, dev) for g in c.grads])
    d_feats = _lib.upload_struct(_feats(c), dev)
    d_off, d_w, d_pos = torch.tensor(c.offsets).to(dev), torch.tensor(c.weights).to(dev), torch.tensor(c.positions).to(dev)
    S = c.D + c.pad
    out = torch.full((c.rows + 1, S), float(ref.SENTINEL), dtype=torch.float32, device=dev)
    gd = grad_dsts(views)
    off_by_one = out.view(-1)[1:]  # 4 bytes behind a 16-byte boundary
    assert out.data_ptr() % 16 == 0 and off_by_one.data_ptr() % 16 == 4

    def call(feats=p(d_feats), n_feats=c.F, off=p(d_off), B=c.B, uniform=0, grads=gd, n_dst=len(views), o=p(out), stride=S, dim=c.D):
        return L.tzr_lookup_grads(feats, n_feats, off, p(d_w), B, uniform, p(d_pos), grads, n_dst, o, stride, dim, st)

    shifted = [w[:, 5:5 + v.shape[1]] for w, v in zip(wides, views)]  # slices from column 5: 4 bytes behind a 16-byte boundary
    assert shifted[1].data_ptr() % 16 == 4
    bad_ptr = grad_dsts([views[0], shifted[1]])
    bad_stride = grad_dsts(views)
    bad_stride[1].stride = views[1].stride(0) + 2
    nine = (_lib.TzrDst * 9)()
    for i in range(9):
        nine[i].ptr, nine[i].stride = gd[i % 2].ptr, gd[i % 2].stride
    refused = {
        "null d_feats": call(feats=None), "n_feats 0": call(n_feats=0), "B < 0": call(B=-1), "n_dst 0": call(n_dst=0),
        "n_dst 9": call(grads=nine, n_dst=9), "dim 0": call(dim=0), "dim 6": call(dim=6, stride=8), "out_stride < dim": call(stride=c.D - 4),
        "out_stride not a multiple of 4": call(stride=S + 2), "ragged bags without offsets": call(off=None),
        "misaligned d_out": call(o=p(off_by_one)), "group pointer not 16-byte aligned": call(grads=bad_ptr),
        "group stride not a multiple of 4": call(grads=bad_stride),
    }
    assert refused == {k: _lib.TZR_ERR_INVALID for k in refused}
    assert call(B=0) == _lib.TZR_OK and call(B=0, uniform=1, off=None) == _lib.TZR_OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), np.full((c.rows + 1, S), SENTINEL_BITS, dtype=np.int32))  # nothing was written
    # ... and the same arguments, unchanged, are a good call
    assert call() == _lib.TZR_OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    _check(c, out.cpu().numpy()[:c.rows], f"abi on {dev.type}")
    del wides, views, shifted, d_feats, d_off, d_w, d_pos, gd, bad_ptr, bad_stride, nine
