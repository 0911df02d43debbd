"""numpy restatement of the norm-based and partial row-wise fused sparse optimizers (include/tzrec_hip.h at
TZR_OPT_PARTIAL_ROWWISE_ADAM): the definition tests/test_sparse_optim_norm.py checks the kernels against.

State rows as the library allocates them: partial row-wise kinds [m(D) | v | pad(3)], LAMB [m(D) | v(D)], LARS-SGD [m(D)].
Duplicate lookups of a row are summed in fp32 in lookup order (as oracle.tzrec_oracle.sparse_update), the update itself is
computed in fp64 and stored as fp32 (fp16 tables: rounded to half)."""
import numpy as np

NORM_KINDS = ("partial_rowwise_adam", "lamb", "partial_rowwise_lamb", "lars_sgd")


def state_width(kind: str, D: int) -> int:
    return {"partial_rowwise_adam": D + 4, "partial_rowwise_lamb": D + 4, "lamb": 2 * D, "lars_sgd": D}[kind]


def summed_rows(ids: np.ndarray, grads: np.ndarray):
    uniq, inv, counts = np.unique(ids, return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind="stable")
    starts = np.zeros(len(uniq), dtype=np.int64)
    np.cumsum(counts[:-1], out=starts[1:])
    return uniq, np.add.reduceat(np.ascontiguousarray(grads, dtype=np.float32)[order], starts, axis=0)


def update_rows(w: np.ndarray, m: np.ndarray, rows: np.ndarray, g: np.ndarray, cfg, step: int) -> None:
    """One update of the rows `rows` (summed gradients g) of weights w [R, D] and state m, in place.  `step` = 1 for the first
    update (the device step counter after the tick); cfg = a SparseOptimizerConfig."""
    if len(rows) == 0:
        return
    D = w.shape[1]
    g = g.astype(np.float32)
    if cfg.gradient_clipping:
        g = np.clip(g, -np.float32(cfg.max_gradient), np.float32(cfg.max_gradient))
    g = g.astype(np.float64)
    x = w[rows].astype(np.float64)
    lr, wd, eps = float(np.float32(cfg.lr)), float(np.float32(cfg.weight_decay)), float(np.float32(cfg.eps))
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


def sparse_update(w: np.ndarray, m: np.ndarray, ids: np.ndarray, grads: np.ndarray, cfg, step: int) -> None:
    """`ids[i]` / `grads[i]` = row and dL/d(row contribution) of lookup i"""
    if len(ids) == 0:
        return
    rows, g = summed_rows(ids, grads)
    update_rows(w, m, rows, g, cfg, step)
