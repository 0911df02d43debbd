"""numpy restatement of every fused sparse optimizer (include/tzrec_hip.h at TZR_OPT_SGD .. TZR_OPT_LARS_SGD, the formulas of
oracle.tzrec_oracle.sparse_update for the first four): the definition tests/test_sparse_optim_norm.py and
tests/test_sparse_dims.py check the kernels against.

State rows as the library allocates them (embedding.EmbeddingBagCollection._allocate), in the canonical form `update_rows`
takes (`unpack` reads them out of any storage layout): Adagrad [m(D)], row-wise Adagrad [m] (one scalar per row), Adam and
LAMB [exp_avg(D) | exp_avg_sq(D)], partial row-wise kinds [m(D) | v | pad(3)], LARS-SGD [m(D)], SGD none.  Duplicate lookups of
a row are summed in fp32 in lookup order (`summed_rows`, as oracle.tzrec_oracle.sparse_update) or in fp64 (`summed_rows64`),
the update itself is computed in fp64 and stored as fp32 (fp16 tables: rounded to half)."""
import numpy as np

NORM_KINDS = ("partial_rowwise_adam", "lamb", "partial_rowwise_lamb", "lars_sgd")
LEGACY_KINDS = ("sgd", "adagrad", "rowwise_adagrad", "adam")
# dyadic upstream gradients: multiples of 2^-DYADIC_BITS (see dyadic_grads)
DYADIC_BITS = 6


def state_width(kind: str, D: int) -> int:
    return {"partial_rowwise_adam": D + 4, "partial_rowwise_lamb": D + 4, "lamb": 2 * D, "lars_sgd": D, "adam": 2 * D,
            "adagrad": D, "rowwise_adagrad": 1, "sgd": 0}[kind]


def new_state(kind: str, rows: int, D: int, init: float = 0.0):
    """the canonical state of a fresh table (None for SGD); `init` = initial_accumulator_value (Adagrad)"""
    if kind == "sgd":
        return None
    if kind == "rowwise_adagrad":
        return np.zeros(rows, np.float32)
    return np.full((rows, state_width(kind, D)), init if kind == "adagrad" else 0.0, np.float32)


def unpack(kind: str, D: int, store: np.ndarray, state):
    """(weights [rows, D], canonical state) out of the storage the library allocated for one table: `store` = the table's
    whole storage tensor (EmbeddingBagCollection._storage), `state` = its separate state tensor or None.  Layouts:
      interleaved Adagrad       store [rows, 2 D] = [w | m]
      interleaved row-wise      store [rows, 2 D] = [w | m | pad(D - 1)], the pad all zero
      split / FP16 / the rest   store [rows, D] = w (fp32 or fp16), state separate (fp32): Adagrad [rows, D], row-wise
                                Adagrad [rows], Adam / LAMB [rows, 2 D], partial row-wise [rows, D + 4], LARS-SGD [rows, D]"""
    store = np.asarray(store)
    if store.shape[1] == 2 * D and kind in ("adagrad", "rowwise_adagrad"):
        assert store.dtype == np.float32
        if kind == "adagrad":
            return store[:, :D], store[:, D:]
        assert not store[:, D + 1:].any(), "the pad behind a row-wise Adagrad scalar was written"
        return store[:, :D], store[:, D].copy()
    assert store.shape[1] == D, store.shape
    if kind == "sgd":
        assert state is None
        return store, None
    state = np.asarray(state)
    assert state.dtype == np.float32
    want = (store.shape[0],) if kind == "rowwise_adagrad" else (store.shape[0], state_width(kind, D))
    assert state.shape == want, (state.shape, want)
    return store, state


def dyadic_grads(rng, shape, sigma: float = 1.0) -> np.ndarray:
    """round(N(0, 1) * 64) / 64 * sigma as fp32 (sigma a power of two): every partial sum of such values is a multiple of
    2^-6 sigma, held exactly in fp32 while its magnitude stays below 2^24 of those steps (assert_exact_sums): the sum of a row's
    gradients is then the same in ANY order, and a kernel's sum must equal the fp64 one bit for bit"""
    assert sigma > 0 and np.log2(sigma) == np.round(np.log2(sigma)), sigma
    return (np.round(rng.standard_normal(shape) * (1 << DYADIC_BITS)) / (1 << DYADIC_BITS) * sigma).astype(np.float32)


def assert_exact_sums(ids: np.ndarray, grads: np.ndarray, sigma: float = 1.0) -> None:
    """the precondition of dyadic_grads' exactness: every gradient is a multiple of q = 2^-6 sigma and, per row,
    sum |g_i| / q < 2^24 (which bounds every partial sum of the row, whatever the order)"""
    g = np.asarray(grads, np.float64) * ((1 << DYADIC_BITS) / sigma)
    assert np.array_equal(g, np.round(g)), "not dyadic"
    if len(ids) == 0:
        return
    _, a = summed_rows64(ids, np.abs(g))
    assert float(a.max()) < 2.0 ** 24, float(a.max())


def summed_rows(ids: np.ndarray, grads: np.ndarray):
    uniq, inv, counts = np.unique(ids, return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind="stable")
    starts = np.zeros(len(uniq), dtype=np.int64)
    np.cumsum(counts[:-1], out=starts[1:])
    return uniq, np.add.reduceat(np.ascontiguousarray(grads, dtype=np.float32)[order], starts, axis=0)


def summed_rows64(ids: np.ndarray, grads: np.ndarray):
    """(distinct rows, their summed gradients) in fp64"""
    uniq, inv = np.unique(ids, return_inverse=True)
    g = np.zeros((len(uniq),) + tuple(np.shape(grads)[1:]), np.float64)
    np.add.at(g, inv, np.asarray(grads, np.float64))
    return uniq, g


def update_rows(w: np.ndarray, m, rows: np.ndarray, g: np.ndarray, cfg, step: int) -> None:
    """One update of the rows `rows` (summed gradients g) of weights w [R, D] and canonical state m, in place.  `step` = 1 for
    the first update (the device step counter after the tick); cfg = a SparseOptimizerConfig.  g in fp64 stays fp64 (a sum of
    summed_rows64); in fp32 it is clipped in fp32 as the kernels do."""
    if len(rows) == 0:
        return
    D = w.shape[1]
    if g.dtype != np.float64:
        g = g.astype(np.float32)
    if cfg.gradient_clipping:
        mg = np.float32(cfg.max_gradient)
        g = np.clip(g, -mg, mg)
    g = g.astype(np.float64)
    x = w[rows].astype(np.float64)
    lr, wd, eps = float(np.float32(cfg.lr)), float(np.float32(cfg.weight_decay)), float(np.float32(cfg.eps))
    if cfg.kind in LEGACY_KINDS:
        _update_legacy(w, m, rows, g, x, cfg, step, lr, wd, eps)
        return
    wn = np.sqrt((x * x).sum(axis=1, keepdims=True))
    if cfg.kind == "lars_sgd":
        mu, eta = float(np.float32(cfg.momentum)), float(np.float32(cfg.eta))
        gn = np.sqrt((g * g).sum(axis=1, keepdims=True))
        den = gn + wd * wn
        lam = np.where(den > 0, lr * eta * wn / np.where(den > 0, den, 1.0), 0.0)
        mm = mu * m[rows, :D].astype(np.float64) + lam * (g + wd * x)
        m[rows, :D] = mm
        w[rows] = (x - mm).astype(w.dtype)
        return
    b1, b2 = float(np.float32(cfg.beta1)), float(np.float32(cfg.beta2))
    c1, c2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    mm = b1 * m[rows, :D].astype(np.float64) + (1 - b1) * g
    if cfg.kind == "lamb":
        v = b2 * m[rows, D:2 * D].astype(np.float64) + (1 - b2) * g * g
        m[rows, D:2 * D] = v
    else:
        v = b2 * m[rows, D:D + 1].astype(np.float64) + (1 - b2) * (g * g).mean(axis=1, keepdims=True)
        m[rows, D] = v[:, 0]
    m[rows, :D] = mm
    u = (mm / c1) / (np.sqrt(v / c2) + eps) + wd * x
    if cfg.kind == "partial_rowwise_adam":
        step_size = lr
    else:
        un = np.sqrt((u * u).sum(axis=1, keepdims=True))
        step_size = np.where(un > 0, lr * wn / np.where(un > 0, un, 1.0), 0.0)
    w[rows] = (x - step_size * u).astype(w.dtype)


def _update_legacy(w, m, rows, g, x, cfg, step, lr, wd, eps) -> None:
    """SGD, Adagrad, row-wise Adagrad (weight-decay modes none / l2 / decouple), Adam: oracle.tzrec_oracle.sparse_update and
    the BWD_FAM_LEGACY / BWD_FAM_ADAM row updates of csrc/pooled_bwd_apply.h"""
    D = w.shape[1]
    if cfg.kind == "sgd":
        w[rows] = (x - lr * g).astype(w.dtype)
    elif cfg.kind == "adagrad":
        mm = m[rows].astype(np.float64) + g * g
        m[rows] = mm
        w[rows] = (x - lr * g / (np.sqrt(mm) + eps)).astype(w.dtype)
    elif cfg.kind == "rowwise_adagrad":
        mode = cfg.weight_decay_mode
        gl = g + wd * x if mode == "l2" else g
        mm = m[rows].astype(np.float64) + (gl * gl).mean(axis=1)
        m[rows] = mm
        mult = (lr / (np.sqrt(mm) + eps))[:, None]
        corr = 1.0 - mult * wd if mode == "l2" else (1.0 - lr * wd if mode == "decouple" else 1.0)
        w[rows] = (corr * x - mult * g).astype(w.dtype)
    else:  # adam: [exp_avg | exp_avg_sq]
        b1, b2 = float(np.float32(cfg.beta1)), float(np.float32(cfg.beta2))
        c1, c2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        ea = b1 * m[rows, :D].astype(np.float64) + (1 - b1) * g
        es = b2 * m[rows, D:2 * D].astype(np.float64) + (1 - b2) * g * g
        m[rows, :D], m[rows, D:2 * D] = ea, es
        w[rows] = (x - lr * ((ea / c1) / (np.sqrt(es / c2) + eps) + wd * x)).astype(w.dtype)


def sparse_update(w: np.ndarray, m: np.ndarray, ids: np.ndarray, grads: np.ndarray, cfg, step: int, fp64: bool = False) -> None:
    """`ids[i]` / `grads[i]` = row and dL/d(row contribution) of lookup i; duplicates summed in fp32 in lookup order, or in
    fp64 (`fp64`)"""
    if len(ids) == 0:
        return
    rows, g = summed_rows64(ids, grads) if fp64 else summed_rows(ids, grads)
    update_rows(w, m, rows, g, cfg, step)
