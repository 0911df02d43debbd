"""Index stage (K1-K4, exchange bucketize) at the sizes where its loops run more than once: the scan's carry over blocks of
tile sums, the grid-stride second passes of permute / bounds check / pad, the `n_out_max` clamp, int64 lengths, rotated owners,
the second batch of tiles of the exchange scan, multi-id bags, W at its limit.  Everything is integer work: bit-exact against
the numpy oracle.  tests/test_index_parity.py holds the small shapes (every loop once or not at all)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle import tzrec_oracle as orc  # noqa: E402
from test_index_parity import _capped_message_from_dense  # noqa: E402
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.embedding import EmbeddingBagCollection, EmbeddingBagConfig  # noqa: E402
from torcheasyrec_amd.sparse import KeyedJaggedTensor, block_bucketize, lengths_to_offsets  # noqa: E402

# the kernels' constants (a changed one fails test_the_shapes_cross_the_thresholds_they_are_meant_for, not silently the coverage)
IDX_THREADS = 256         # csrc/index_ops.hip:12
IDX_TILE = 2048           # csrc/index_ops.hip:14  IDX_THREADS * IDX_ITEMS
PERM_LEN_GRID = 64        # csrc/index_ops.hip:225 gx cap of tzr_permute_lengths_kernel
PERM_VAL_GRID = 128       # csrc/index_ops.hip:233 grid.x of tzr_permute_values_kernel
BOUNDS_GRID = 256         # csrc/index_ops.hip:164 gx cap of tzr_bounds_check_kernel
XB_THREADS = 256          # csrc/index_ops.hip:349
XB_TILE = 1024            # csrc/index_ops.hip:350
XB_SCAN_BATCH = 16        # csrc/index_ops.hip:404 tiles per batch of independent loads in tzr_xb_scan_kernel
XB_MAX_W = 64             # csrc/index_ops.hip:528 lanes of cnt[64], 6 ballot bits
XB_PAD_GRID = 4096        # csrc/index_ops.hip:642 grid cap of tzr_xb_pad_kernel

SCAN_ONE_PASS = IDX_THREADS * IDX_TILE  # lengths one pass of tzr_scan_tile_prefix_kernel's carry loop covers
SCAN_NS = [SCAN_ONE_PASS, SCAN_ONE_PASS + 1, 2 * SCAN_ONE_PASS + 5]
PERMUTE_LARGE = (3, 17_000, 5)  # F, B, longest bag
BUCKETIZE_SHAPES = [(3, 700, 8, 6), (3, 22_000, 8, 2)]  # F, B, W, longest bag
BOUNDS_SHAPES = [(300, 20), (66_000, 3)]  # B, longest bag
EXCHANGE_SHAPES = [(8, 16_500, 1), (8, 16_500, 2), (64, 1_100, 1), (33, 1_100, 3)]  # W, B, bag_len
PAD_LARGE = (4, 3, 350_000)  # W, F, B
ROWS = [1000, 17, 40_000_000]


def test_the_shapes_cross_the_thresholds_they_are_meant_for():
    # scan: exactly one pass of the carry loop, one element into the second, into the third
    assert [(n + IDX_TILE - 1) // IDX_TILE for n in SCAN_NS] == [IDX_THREADS, IDX_THREADS + 1, 2 * IDX_THREADS + 1]
    F, B, max_len = PERMUTE_LARGE
    assert B > PERM_LEN_GRID * IDX_THREADS  # tzr_permute_lengths_kernel strides
    assert B * max_len / 2 > PERM_VAL_GRID * IDX_THREADS  # the expected ids of a key (asserted on the drawn ones in the test)
    assert 4 * B > IDX_TILE  # its scan: more than one tile
    (f0, b0, w0, _), (f1, b1, w1, _) = BUCKETIZE_SHAPES
    assert IDX_TILE < w0 * f0 * b0 <= SCAN_ONE_PASS and (w0 * f0 * b0 + IDX_TILE - 1) // IDX_TILE == 9
    assert 22_000 * 3 * 8 > 256 * IDX_TILE and w1 * f1 * b1 > SCAN_ONE_PASS  # the scan's carry loop runs
    assert f0 == f1 == len(ROWS) and -(-ROWS[1] // w0) * (w0 - 2) >= ROWS[1]  # 17 rows over 8 ranks: the last ranks own nothing
    (bs, ls), (bl, ll) = BOUNDS_SHAPES
    assert (bs + IDX_THREADS - 1) // IDX_THREADS == 2 and bs * ls / 2 > 4 * 2 * IDX_THREADS  # two workgroups, several passes
    assert (bl + IDX_THREADS - 1) // IDX_THREADS > BOUNDS_GRID and bl * ll / 2 > BOUNDS_GRID * IDX_THREADS  # gx capped, and strides
    tiles = [(B * L + XB_TILE - 1) // XB_TILE for _, B, L in EXCHANGE_SHAPES]
    assert 16_500 > 16 * XB_TILE and tiles[0] == XB_SCAN_BATCH + 1 and tiles[1] == 2 * XB_SCAN_BATCH + 1
    assert EXCHANGE_SHAPES[1][2] > 1 and EXCHANGE_SHAPES[3][2] > 1  # bags of more than one id
    assert EXCHANGE_SHAPES[2][0] == XB_MAX_W and EXCHANGE_SHAPES[2][0] * 3 <= XB_THREADS
    w = EXCHANGE_SHAPES[3][0]
    assert w > 32 and w & (w - 1) and tiles[3] > 1  # a large non-power of two: 6 ballot bits, codes 33..63 unused
    assert all((B * L) % XB_TILE for _, B, L in EXCHANGE_SHAPES)  # ragged last tiles
    W, F, B = PAD_LARGE
    assert XB_PAD_GRID * XB_THREADS < F * B < 2 * XB_PAD_GRID * XB_THREADS and W <= XB_MAX_W


# ---- K3 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SCAN_NS)
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_lengths_to_offsets_carries_across_blocks_of_tile_sums(dev, n, dtype):
    rng = np.random.default_rng(n)
    lengths = torch.from_numpy(rng.integers(0, 9, size=n)).to(dtype)
    d_len = lengths.to(dev)
    got = lengths_to_offsets(d_len).cpu().numpy()
    ref = orc.lengths_to_offsets(lengths.numpy())
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert np.array_equal(lengths_to_offsets(d_len).cpu().numpy(), got)  # deterministic


# ---- K1 ---------------------------------------------------------------------------------------------------------------

def _ragged_kjt(rng, F, B, max_len, rows, weighted, dtype):
    lens = rng.integers(0, max_len + 1, size=F * B).astype(dtype)
    lens[rng.integers(0, F * B, size=F)] = 0
    vals = rng.integers(0, rows, size=int(lens.sum())).astype(np.int64)
    w = rng.uniform(0, 1, size=len(vals)).astype(np.float32) if weighted else None
    return [f"k{i}" for i in range(F)], vals, lens, w


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_kjt_permute_strides_over_samples_and_ids(dev, dtype):
    """More samples than tzr_permute_lengths_kernel's grid covers at once, more ids per key than tzr_permute_values_kernel's,
    a key taken twice, 34 scan tiles, weights, both length widths."""
    rng = np.random.default_rng(17)
    F, B, max_len = PERMUTE_LARGE
    perm = [2, 0, 2, 1]
    keys, vals, lens, w = _ragged_kjt(rng, F, B, max_len, 1 << 40, True, dtype)
    assert lens.reshape(F, B).sum(1).min() > PERM_VAL_GRID * IDX_THREADS
    kjt = KeyedJaggedTensor(keys, torch.from_numpy(vals), torch.from_numpy(lens), torch.from_numpy(w)).to(dev)
    out = kjt.permute(perm)
    rl, rv, rw = orc.kjt_permute(perm, lens, vals, w, B)
    assert out.keys() == [keys[i] for i in perm]
    got_l = out.lengths().cpu().numpy()
    assert got_l.dtype == dtype and np.array_equal(got_l, rl)
    assert np.array_equal(out.offsets().cpu().numpy(), orc.lengths_to_offsets(rl))
    assert np.array_equal(out.values().cpu().numpy(), rv)
    assert np.array_equal(out.weights().cpu().numpy(), rw)


def _permute_entry(dev, perm, F, B, lens, in_off, vals, w, n_alloc, n_out_max, sentinel=-7):
    """tzr_kjt_permute called directly; output buffers pre-filled with `sentinel`"""
    T = len(perm)
    d = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_perm, d_lens, d_off, d_vals, d_w = d(np.asarray(perm, np.int32)), d(lens), d(in_off), d(vals), d(w)
    out_l = torch.full((max(T * B, 1),), sentinel, dtype=d_lens.dtype, device=dev)
    out_o = torch.full((T * B + 1,), sentinel, dtype=torch.int64, device=dev)
    out_v = torch.full((max(n_alloc, 1),), sentinel, dtype=torch.int64, device=dev)
    out_w = torch.full((max(n_alloc, 1),), float(sentinel), dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.tzr_kjt_permute_workspace(T, B), dev)
    rc = L.tzr_kjt_permute(_lib.ptr(d_perm), T, F, B, _lib.ptr(d_lens), d_lens.element_size(), _lib.ptr(d_off), _lib.ptr(d_vals), _lib.ptr(d_w),
                           _lib.ptr(out_l), _lib.ptr(out_o), _lib.ptr(out_v), _lib.ptr(out_w), n_out_max, _lib.ptr(ws), ws.numel(),
                           _lib.stream_ptr(dev))
    return rc, out_l.cpu().numpy(), out_o.cpu().numpy(), out_v.cpu().numpy(), out_w.cpu().numpy()


def test_kjt_permute_stops_at_n_out_max(dev):
    """An output smaller than the sum of the selected keys (a caller that sized it from a hint): the last key is cut in half,
    nothing at or behind `n_out_max` is written; lengths and offsets are those of the whole permutation."""
    rng = np.random.default_rng(3)
    F, B, perm = 3, 700, [2, 0, 1]
    _, vals, lens, w = _ragged_kjt(rng, F, B, 5, 1 << 40, True, np.int32)
    in_off = orc.lengths_to_offsets(lens)
    rl, rv, rw = orc.kjt_permute(perm, lens, vals, w, B)
    ro = orc.lengths_to_offsets(rl)
    last = int(ro[2 * B])
    n_max = last + (len(rv) - last) // 2
    assert last + IDX_THREADS < n_max < len(rv) - IDX_THREADS  # the cut falls inside the last key, workgroups on both sides
    rc, gl, go, gv, gw = _permute_entry(dev, perm, F, B, lens, in_off, vals, w, len(rv), n_max)
    assert rc == _lib.TZR_OK
    assert np.array_equal(gl, rl) and np.array_equal(go, ro)
    assert np.array_equal(gv[:n_max], rv[:n_max]) and np.array_equal(gw[:n_max], rw[:n_max])
    assert (gv[n_max:] == -7).all() and (gw[n_max:] == -7.0).all()
    # a cut in front of the last key: that key writes nothing at all
    n_max = last - 5
    rc, gl, go, gv, gw = _permute_entry(dev, perm, F, B, lens, in_off, vals, w, len(rv), n_max)
    assert rc == _lib.TZR_OK and np.array_equal(go, ro)
    assert np.array_equal(gv[:n_max], rv[:n_max]) and (gv[n_max:] == -7).all() and (gw[n_max:] == -7.0).all()


def test_kjt_permute_of_an_empty_batch(dev):
    z = np.zeros(0, np.int64)
    rc, gl, go, gv, gw = _permute_entry(dev, [1, 0], 3, 0, np.zeros(0, np.int32), np.zeros(1, np.int64), z, np.zeros(0, np.float32), 0, 0)
    assert rc == _lib.TZR_OK
    assert go.tolist() == [0]
    assert (gl == -7).all() and (gv == -7).all() and (gw == -7.0).all()  # nothing else is touched


# ---- K2 ---------------------------------------------------------------------------------------------------------------

def _edge_ids(rows, W):
    """first and last id of every rank's block, last row of the table"""
    block = -(-rows // W)
    e = [0, rows - 1] + [r * block + k for r in range(1, W) for k in (-1, 0)]
    return np.array(sorted({x for x in e if 0 <= x < rows}), dtype=np.int64)


@pytest.mark.parametrize("weighted,rotated,hashed", [(False, False, False), (True, False, False), (False, True, False), (True, True, False),
                                                     (True, True, True)])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("F,B,W,max_len", BUCKETIZE_SHAPES)
def test_block_bucketize_over_many_scan_tiles(dev, F, B, W, max_len, dtype, weighted, rotated, hashed):
    """W*F*B bag lengths of 9 scan tiles, and of more than one pass of the scan's carry loop; both length widths; owners
    rotated per key (compared with the ORACLE, not with the sibling kernel); ids on both sides of every block edge."""
    rng = np.random.default_rng(B + W + 2 * weighted + rotated)
    lens = rng.integers(0, max_len + 1, size=F * B).astype(dtype)
    lens[rng.integers(0, F * B, size=F)] = 0
    off = orc.lengths_to_offsets(lens)
    block = np.array([-(-r // W) for r in ROWS], dtype=np.int64)  # ceil(rows / W)
    vals = np.empty(int(off[-1]), dtype=np.int64)
    for f in range(F):
        seg = vals[off[f * B]:off[(f + 1) * B]]
        seg[:] = rng.integers(0, ROWS[f], size=len(seg))
        edges = _edge_ids(ROWS[f], W)
        assert len(seg) > 4 * len(edges)
        seg[rng.choice(len(seg), size=len(edges), replace=False)] = edges
    if hashed:  # key 1 routed by the hash of raw 64-bit ids
        block[1] = 0
        seg = vals[off[B]:off[2 * B]]
        seg[:] = rng.integers(-(1 << 62), 1 << 62, size=len(seg))
        seg[:3] = [0, -1, (1 << 63) - 2]
    w = rng.uniform(0, 1, size=len(vals)).astype(np.float32) if weighted else None
    rot = np.array([1 % W, 0, W - 1], dtype=np.int32) if rotated else None
    kjt = KeyedJaggedTensor([f"k{i}" for i in range(F)], torch.from_numpy(vals), torch.from_numpy(lens),
                            torch.from_numpy(w) if weighted else None).to(dev)
    out, unb = block_bucketize(kjt, torch.from_numpy(block).to(dev), W, return_permute=True,
                               rank_offsets=torch.from_numpy(rot).to(dev) if rotated else None)
    rl, rv, rw, ru = orc.block_bucketize(block, lens, vals, w, B, W, rot)
    got_l = out.lengths().cpu().numpy()
    assert got_l.dtype == dtype and np.array_equal(got_l, rl)
    assert np.array_equal(out.offsets().cpu().numpy(), orc.lengths_to_offsets(rl))
    assert np.array_equal(out.values().cpu().numpy(), rv)
    assert np.array_equal(unb.cpu().numpy(), ru)
    if weighted:
        assert np.array_equal(out.weights().cpu().numpy(), rw)
    # the reference itself: key 1 (17 rows in blocks of 3, never rotated) fills ranks 0..5 only; key 0's rotation by one rank
    # moves its id 0 from rank 0 to rank 1
    per = rl.reshape(W, F, B).astype(np.int64).sum(2)
    if not hashed:
        assert (per[:6, 1] > 0).all() and (per[6:, 1] == 0).all()
    rank_start = orc.lengths_to_offsets(rl)[::F * B]
    where_id0 = ru[np.flatnonzero(vals[:off[B]] == 0)[0]]
    assert np.searchsorted(rank_start, where_id0, side="right") - 1 == (1 if rotated else 0)


# ---- K4 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [_lib.BOUNDS_FATAL, _lib.BOUNDS_WARNING, _lib.BOUNDS_IGNORE])
@pytest.mark.parametrize("B,max_len", BOUNDS_SHAPES)
def test_bounds_check_strides_over_a_keys_ids(dev, B, max_len, mode):
    rng = np.random.default_rng(B)
    ebc = EmbeddingBagCollection([EmbeddingBagConfig("t0", 16, 10, ["a"]), EmbeddingBagConfig("t1", 16, 1000, ["b"])], device=dev)
    lens = rng.integers(0, max_len + 1, size=2 * B).astype(np.int32)
    off = orc.lengths_to_offsets(lens)
    gx = min(BOUNDS_GRID, (B + IDX_THREADS - 1) // IDX_THREADS)
    assert min(off[B], off[2 * B] - off[B]) > gx * IDX_THREADS  # a second pass for both keys
    vals = np.concatenate([rng.integers(-2, 14, size=int(off[B])), rng.integers(990, 1010, size=int(off[2 * B] - off[B]))]).astype(np.int64)
    vals[[0, off[B] - 1, off[B], -1]] = [-1, 10, 1000, 1 << 40]  # first and last id of each key out of range
    kjt = KeyedJaggedTensor(["a", "b"], torch.from_numpy(vals.copy()), torch.from_numpy(lens)).to(dev)
    cnt = ebc.bounds_check(kjt, mode)
    ref_vals, ref_bad = orc.bounds_check(vals, off, [10, 1000], B, clamp=mode != _lib.BOUNDS_FATAL)
    assert ref_bad > 1000
    assert int(cnt.item()) == (0 if mode == _lib.BOUNDS_IGNORE else ref_bad)
    assert np.array_equal(kjt.values().cpu().numpy(), ref_vals)


# ---- exchange bucketize ---------------------------------------------------------------------------------------------------

def _exchange_inputs(rng, W, B, bag_len, hashed):
    rows = [1000, 17, 40_000_000, 300, 9]
    sel = [3, 1, 2]  # a subset, reordered
    n_per_key = B * bag_len
    vals = np.stack([rng.integers(0, rows[f], size=n_per_key) for f in range(5)]).astype(np.int64)
    block = np.array([-(-rows[f] // W) for f in sel], dtype=np.int64)
    if hashed:
        vals[1] = rng.integers(-(1 << 62), 1 << 62, size=n_per_key)
        block[1] = 0  # key k1 routed by hash
    rot = np.array([1 % W, 0, W - 1], dtype=np.int32)
    return sel, vals.reshape(-1), block, rot


def _exchange_oracle(sel, vals, block, rot, B, bag_len, W):
    """K1 + K2 of the oracle on the uniform bags: ids by (rank, key) in lookup order, positions, counts"""
    lens = np.full(5 * B, bag_len, dtype=np.int32)
    pl, pv, _ = orc.kjt_permute(sel, lens, vals, None, B)
    nl, nv, _, nu = orc.block_bucketize(block, pl, pv, None, B, W, rot)
    return nv, nu, nl.reshape(W * len(sel), B).astype(np.int64).sum(1)


@pytest.mark.parametrize("W,B,bag_len", EXCHANGE_SHAPES)
def test_exchange_bucketize_matches_the_oracle(dev, W, B, bag_len):
    """17 and 33 tiles per key (the second and third batch of the one-workgroup scan), bags of 2 and 3 ids, 64 ranks (every lane of
    the counters, all 6 ballot bits), 33 ranks with a hashed key: the dense form, the capacity-bounded form at a capacity that
    fits and one that does not, the same layout from the dense result, the owner's key segments -- all against the oracle."""
    rng = np.random.default_rng(W * 7 + bag_len)
    sel, vals, block, rot = _exchange_inputs(rng, W, B, bag_len, hashed=W == 33)
    F, n_per_key = len(sel), B * bag_len
    n = F * n_per_key
    want_ids, want_unb, want_cnt = _exchange_oracle(sel, vals, block, rot, B, bag_len, W)
    L = _lib.lib()
    d = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_vals, d_blk, d_rot, d_sel = d(vals), d(block), d(rot), d(np.asarray(sel, np.int32))
    ws = _lib.workspace(L.tzr_exchange_bucketize_workspace(F, n_per_key, W), dev)

    def dense():
        out = torch.full((n,), -7, dtype=torch.int64, device=dev)
        unb = torch.full((n,), -7, dtype=torch.int64, device=dev)
        cnt = torch.full((W * F,), -7, dtype=torch.int64, device=dev)
        _lib.check(L.tzr_exchange_bucketize(_lib.ptr(d_sel), F, _lib.ptr(d_blk), _lib.ptr(d_rot), B, bag_len, W, _lib.ptr(d_vals),
                                            _lib.ptr(out), _lib.ptr(unb), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
                   "tzr_exchange_bucketize")
        return out, unb, cnt

    out, unb, cnt = dense()
    assert np.array_equal(cnt.cpu().numpy(), want_cnt)
    assert np.array_equal(unb.cpu().numpy(), want_unb)
    assert np.array_equal(out.cpu().numpy(), want_ids)
    again = dense()
    assert all(torch.equal(a, b) for a, b in zip(again, (out, unb, cnt)))  # deterministic

    per_dest = want_cnt.reshape(W, F).sum(1)
    assert per_dest.max() >= 2
    for cap, overflows in ((int(per_dest.max()), False), (max(1, int(per_dest.max()) // 2), True)):
        assert bool((per_dest > cap).any()) == overflows
        S = L.tzr_exchange_message_stride(F, cap)
        assert S == F + 1 + cap
        want_msg, want_unb2, want_over = _capped_message_from_dense(want_ids, want_unb, want_cnt, W, F, cap)
        assert want_over == int(overflows)
        msg = torch.full((W * S,), -7, dtype=torch.int64, device=dev)
        unb2 = torch.full((n,), -7, dtype=torch.int64, device=dev)
        _lib.check(L.tzr_exchange_bucketize_capped(_lib.ptr(d_sel), F, _lib.ptr(d_blk), _lib.ptr(d_rot), B, bag_len, W, _lib.ptr(d_vals),
                                                   cap, _lib.ptr(msg), _lib.ptr(unb2), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
                   "tzr_exchange_bucketize_capped")
        assert np.array_equal(msg.cpu().numpy(), want_msg)
        assert np.array_equal(unb2.cpu().numpy(), want_unb2)
        # the same layout from the dense result (the path ragged / weighted bags take)
        msg3 = torch.full((W * S,), -7, dtype=torch.int64, device=dev)
        unb3 = torch.full((n,), -7, dtype=torch.int64, device=dev)
        _lib.check(L.tzr_exchange_pad(_lib.ptr(cnt), W, F, cap, _lib.ptr(out), _lib.ptr(unb), n, _lib.ptr(msg3), _lib.ptr(unb3),
                                      _lib.stream_ptr(dev)), "tzr_exchange_pad")
        assert np.array_equal(msg3.cpu().numpy(), want_msg) and np.array_equal(unb3.cpu().numpy(), want_unb2)
        # owner side (a world where every rank sent this very message): key segments + the flag
        ks = torch.full((W * (F + 1) + 2,), -1, dtype=torch.int64, device=dev)
        flag = torch.full((1,), -1, dtype=torch.int64, device=dev)
        _lib.check(L.tzr_exchange_owner_segments(_lib.ptr(msg), W, F, cap, _lib.ptr(ks), _lib.ptr(flag), _lib.stream_ptr(dev)),
                   "tzr_exchange_owner_segments")
        assert int(flag.item()) == want_over
        want_ks = np.empty(W * (F + 1) + 2, dtype=np.int64)
        hdr = want_msg.reshape(W, S)[:, :F]
        starts = (np.arange(W) * S + F + 1)[:, None] + np.concatenate([np.zeros((W, 1), np.int64), np.cumsum(hdr, 1)], 1)  # [W, F + 1]
        want_ks[1:W * (F + 1) + 1] = starts.reshape(-1)  # a rank's F keys, then the dead key that starts where its ids end
        want_ks[0], want_ks[-1] = 0, W * S
        # (laid out as [dead, key 0 .. key F-1] per rank: the dead key of rank s starts where rank s - 1's ids end)
        assert np.array_equal(ks.cpu().numpy(), want_ks)


def test_exchange_entries_refuse_more_ranks_or_segments_than_they_hold(dev):
    L = _lib.lib()
    B, cap = 8, 4

    def entries(W, F):
        n = F * B
        z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
        sel, blk, rot, vals = torch.arange(F, dtype=torch.int32).to(dev), z(F) + 1, z(F, torch.int32), z(n)
        out, unb, unb2, unb3, cnt, msg, msg3 = z(n), z(n), z(n), z(n), z(W * F), z(W * (F + 1 + cap)), z(W * (F + 1 + cap))
        ks, flag = z(W * (F + 1) + 2), z(1)
        ws = _lib.workspace(L.tzr_exchange_bucketize_workspace(F, B, W), dev)
        p, s = _lib.ptr, _lib.stream_ptr(dev)
        return (L.tzr_exchange_bucketize(p(sel), F, p(blk), p(rot), B, 1, W, p(vals), p(out), p(unb), p(cnt), p(ws), ws.numel(), s),
                L.tzr_exchange_bucketize_capped(p(sel), F, p(blk), p(rot), B, 1, W, p(vals), cap, p(msg), p(unb2), p(ws), ws.numel(), s),
                L.tzr_exchange_pad(p(cnt), W, F, cap, p(out), p(unb), n, p(msg3), p(unb3), s),
                L.tzr_exchange_owner_segments(p(msg), W, F, cap, p(ks), p(flag), s))

    U = _lib.TZR_ERR_UNSUPPORTED
    assert entries(XB_MAX_W + 1, 1) == (U, U, U, U)
    assert XB_MAX_W * 5 > XB_THREADS
    assert entries(XB_MAX_W, 5)[:2] == (U, U)  # one (rank, key) segment per lane of the scan's workgroup
    assert entries(XB_MAX_W, 4) == (_lib.TZR_OK,) * 4  # exactly at both limits: taken


def test_exchange_pad_strides_over_the_ids(dev):
    """More lookups than tzr_xb_pad_kernel's grid covers at once, from a dense bucketize result built on the host."""
    rng = np.random.default_rng(9)
    W, F, B = PAD_LARGE
    n = F * B
    slot = rng.integers(0, W, size=n) * F + np.repeat(np.arange(F), B)  # (dest, key) of every lookup
    order = np.argsort(slot, kind="stable")
    unb = np.empty(n, dtype=np.int64)
    unb[order] = np.arange(n)
    ids = rng.integers(0, 1 << 40, size=n).astype(np.int64)
    cnt = np.bincount(slot, minlength=W * F).astype(np.int64)
    per_dest = cnt.reshape(W, F).sum(1)
    L = _lib.lib()
    d_cnt, d_ids, d_unb = (torch.from_numpy(a).to(dev) for a in (cnt, ids, unb))
    for cap, overflows in ((int(per_dest.max()), False), (int(per_dest.max()) // 2, True)):
        S = F + 1 + cap
        want_msg, want_unb, want_over = _capped_message_from_dense(ids, unb, cnt, W, F, cap)
        assert want_over == int(overflows)
        msg = torch.full((W * S,), -7, dtype=torch.int64, device=dev)
        unb2 = torch.full((n,), -7, dtype=torch.int64, device=dev)
        _lib.check(L.tzr_exchange_pad(_lib.ptr(d_cnt), W, F, cap, _lib.ptr(d_ids), _lib.ptr(d_unb), n, _lib.ptr(msg), _lib.ptr(unb2),
                                      _lib.stream_ptr(dev)), "tzr_exchange_pad")
        assert np.array_equal(msg.cpu().numpy(), want_msg)
        assert np.array_equal(unb2.cpu().numpy(), want_unb)
