"""numpy restatement of the two elementwise sparse optimizers without a step counter, Adadelta and RMSprop
(include/tzrec_hip.h at TZR_OPT_ADADELTA): "lazy" torch.optim.Adadelta / torch.optim.RMSprop (momentum 0, not centered) -- a
row is updated only in a step that looks it up.  fbgemm has no public kernel for either kind, so this file IS the
definition the kernels are checked against; tests/test_sparse_optim_elem.py pins it to the two torch optimizers.

Per touched row, g = its summed (then clipped) gradient, w = its weights before the update:
    g = g + wd w
    rmsprop:   s = alpha s + (1 - alpha) g^2;  w -= lr g / (sqrt(s) + eps)
    adadelta:  s = rho s + (1 - rho) g^2;  d = sqrt(a + eps) / sqrt(s + eps) g;  a = rho a + (1 - rho) d^2;  w -= lr d
State rows as the library allocates them: rmsprop [s(D)], adadelta [s(D) | a(D)], fp32, zero at the start.  The update is
computed in `dtype` (fp64: the reference; fp32: the reference-against-reference check of a test's inputs) and stored as
fp32 (fp16 tables: rounded to half)."""
import numpy as np

from sparse_optim_ref import summed_rows, summed_rows64

ELEM_KINDS = ("adadelta", "rmsprop")


def state_width(kind: str, D: int) -> int:
    return {"adadelta": 2 * D, "rmsprop": D}[kind]


def decay_of(cfg) -> float:
    return cfg.rho if cfg.kind == "adadelta" else cfg.alpha


def update_rows(w: np.ndarray, m: np.ndarray, rows: np.ndarray, g: np.ndarray, cfg, dtype=np.float64) -> None:
    """One update of the rows `rows` (summed gradients g) of weights w [R, D] and state m [R, state_width], in place.  g in
    fp64 stays fp64 (a sum of summed_rows64); in fp32 it is clipped in fp32 as the kernels do."""
    if len(rows) == 0:
        return
    D = w.shape[1]
    if g.dtype != np.float64:
        g = g.astype(np.float32)
    if cfg.gradient_clipping:
        mg = np.float32(cfg.max_gradient)
        g = np.clip(g, -mg, mg)
    T = dtype
    g = g.astype(T)
    x = w[rows].astype(T)
    lr, wd, eps, rho = (T(np.float32(v)) for v in (cfg.lr, cfg.weight_decay, cfg.eps, decay_of(cfg)))
    one = T(1.0)
    g = g + wd * x
    s = rho * m[rows, :D].astype(T) + (one - rho) * g * g
    m[rows, :D] = s
    if cfg.kind == "rmsprop":
        w[rows] = (x - lr * g / (np.sqrt(s) + eps)).astype(w.dtype)
        return
    a = m[rows, D:2 * D].astype(T)
    d = np.sqrt(a + eps) / np.sqrt(s + eps) * g
    m[rows, D:2 * D] = rho * a + (one - rho) * d * d
    w[rows] = (x - lr * d).astype(w.dtype)


def sparse_update(w: np.ndarray, m: np.ndarray, ids: np.ndarray, grads: np.ndarray, cfg, fp64: bool = False, dtype=np.float64) -> None:
    """`ids[i]` / `grads[i]` = row and dL/d(row contribution) of lookup i; duplicates summed in fp32 in lookup order, or in
    fp64 (`fp64`)"""
    if len(ids) == 0:
        return
    rows, g = summed_rows64(ids, grads) if fp64 else summed_rows(ids, grads)
    update_rows(w, m, rows, g, cfg, dtype)
