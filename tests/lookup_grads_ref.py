"""Inputs and the float64 restatement of tzr_lookup_grads (csrc/sharded_ops.hip) for tests/test_lookup_grads.py.

For id i of bag (key f, sample b) with bounds st..en:
    out[pos(i), 0:D] = (w_i or 1) * (1/(en-st) if mean and en-st > 1 else 1) * sum_groups grad_g[b, col_g(f) : col_g(f)+D]
with pos(i) = positions[i], or i when there are no positions.  Plain loops over bags; no library call.

A case is drawn once per set of arguments and shared by every test that asks for it (emulator and device alike); its arrays are
read-only."""
import functools

import numpy as np

SENTINEL = np.float32(-7.25)  # what the output holds before the call: rows nobody addresses and columns >= D keep it bit for bit
MAX_FEAT_DST = 4  # TZR_MAX_FEAT_DST
EPS = 2.0 ** -24  # one rounding to fp32


class Case:
    pass


@functools.lru_cache(maxsize=None)
def draw(B, F, D, G, ragged=True, weighted=False, permuted=False, extra=0, pad=0, seed=0, n_dst=None, pooling=None, dyadic=False):
    """One call's host inputs, the float64 result and the per-element bound.

    Lookup f draws its own number of groups (1..min(4, G), or inside `n_dst` = (lo, hi)), its own distinct groups and its own
    pooling (or `pooling` for all); columns are handed out per group cumulatively, so two lookups read different offsets of a
    group; `key` is a permutation of the lookup index.  `dyadic`: gradients k/64, weights in {0.5, 1, 2}, bag lengths in
    {1, 2, 4} -- every operation of the kernel is exact."""
    rng = np.random.default_rng([B, F, D, G, int(ragged), int(weighted), int(permuted), extra, pad, seed])
    c = Case()
    c.B, c.F, c.D, c.G, c.ragged, c.extra, c.pad = B, F, D, G, ragged, extra, pad
    c.key = rng.permutation(F).astype(np.int32)
    if F > 1 and np.array_equal(c.key, np.arange(F)):
        c.key = np.roll(c.key, 1)  # never the identity
    lo, hi = n_dst if n_dst is not None else (1, min(MAX_FEAT_DST, G))
    c.n_dst = rng.integers(lo, hi + 1, size=F).astype(np.int32)
    c.pool = (rng.integers(0, 2, size=F) if pooling is None else np.full(F, pooling)).astype(np.int32)
    if pooling is None:
        c.pool[0] = 1  # a mean lookup for the length-1 bag below, and, with two lookups, both poolings
        if F > 1:
            c.pool[1] = 0
    c.dst = np.zeros((F, MAX_FEAT_DST), dtype=np.int32)
    c.col = np.zeros((F, MAX_FEAT_DST), dtype=np.int32)
    width = np.zeros(G, dtype=np.int64)
    for f in range(F):
        c.dst[f, :c.n_dst[f]] = rng.choice(G, size=c.n_dst[f], replace=False)
        for d in range(c.n_dst[f]):
            g = c.dst[f, d]
            c.col[f, d] = width[g]
            width[g] += D
    c.width = np.maximum(width, D)  # (a group no lookup reads still needs an address)
    if dyadic:
        c.grads = [(rng.integers(-32, 33, size=(B, int(w))) / 64.0).astype(np.float32) for w in c.width]
    else:
        c.grads = [rng.standard_normal((B, int(w))).astype(np.float32) for w in c.width]
    # bags
    if ragged:
        lens = rng.choice([1, 2, 4], size=F * B) if dyadic else rng.integers(0, 5, size=F * B)
        if not dyadic:
            if F * B == 1:
                lens[0] = 3  # the smallest case still divides
            else:
                lens[int(c.key[0]) * B] = 1  # a mean bag of one id: no divide
                lens[int(c.key[F - 1]) * B + B - 1] = 0  # an empty bag: skipped
    else:
        lens = np.ones(F * B, dtype=np.int64)
    c.lens = lens.astype(np.int64)
    c.offsets = np.concatenate([[0], np.cumsum(c.lens)]).astype(np.int64)
    c.N = int(c.offsets[-1])
    if not weighted:
        c.weights = None
    elif dyadic:
        c.weights = rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=c.N)
    else:
        c.weights = rng.uniform(0.5, 1.5, size=c.N).astype(np.float32)
    c.rows = max(c.N + extra, 1)
    c.positions = rng.permutation(c.N + extra)[:c.N].astype(np.int64) if permuted else None
    # float64 on the fp32 inputs
    c.want = np.full((c.rows, D + pad), float(SENTINEL), dtype=np.float64)
    c.bound = np.zeros((c.rows, D + pad), dtype=np.float64)
    c.written = np.zeros(c.rows, dtype=bool)
    g64 = [g.astype(np.float64) for g in c.grads]
    for f in range(F):
        k, n = int(c.key[f]), int(c.n_dst[f])
        for b in range(B):
            st, en = int(c.offsets[k * B + b]), int(c.offsets[k * B + b + 1])
            if st >= en:
                continue
            total, mag = np.zeros(D), np.zeros(D)
            for d in range(n):
                piece = g64[c.dst[f, d]][b, c.col[f, d]:c.col[f, d] + D]
                total, mag = total + piece, mag + np.abs(piece)
            inv = 1.0 / (en - st) if c.pool[f] == 1 and en - st > 1 else 1.0
            for i in range(st, en):
                scale = (float(c.weights[i]) if c.weights is not None else 1.0) * inv
                p = int(c.positions[i]) if c.positions is not None else i
                assert not c.written[p]
                c.want[p, :D] = scale * total
                # n - 1 additions, the reciprocal, w * inv and the product: each rounded once to fp32
                c.bound[p, :D] = (n + 2) * EPS * mag * abs(scale)
                c.written[p] = True
    for a in [c.key, c.n_dst, c.pool, c.dst, c.col, c.lens, c.offsets, c.want, c.bound, c.written, *c.grads] + \
            [x for x in (c.weights, c.positions) if x is not None]:
        a.setflags(write=False)
    return c
