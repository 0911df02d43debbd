"""The fused sparse backward at every embedding dim the collection takes a table of, not only D = 16: every apply kernel gives a
row D / 4 lanes and packs 64 / (D / 4) lookups into a tile, and what happens at a group size that is not a power of two
(D = 12, 20, 24, 40, 48: idle tail lanes, the other branch of bwd_group_sum, the `gi + d < gw` guard of the direct kernel's
tree reduce), at 2 or 1 lookups per tile (D = 128, 256) and beside a max_dim of 256 (split-row records and row-split partial
sums are indexed by max_dim) runs nowhere else.  Against the float64 restatement of tests/sparse_optim_ref.py.

Tolerances.  Most cases draw DYADIC upstream gradients (sparse_optim_ref.dyadic_grads: multiples of 2^-6, every partial sum
exact in fp32, asserted): the summed gradient of a row is then the same in every order, and what is left between a kernel and
float64 is the fp32 arithmetic of one row update -- a few ulp -- checked at `rtol=2e-5, atol=1e-7` (EXACT).  The gradients are
scaled by a power of two (_sigma) so that summed rows stay O(1): Adam's exp_avg = b1 m + (1 - b1) g cancels, and its
result carries an ulp of its OPERANDS (FMA or not), which atol = 1e-7 covers only while they stay below ~1.  Every step starts
the reference from the library's own state before that step, so each step is checked on its own.  fp16 tables: the half-ulp
rule of test_pooled_parity.test_fp16_tables.  Jagged, weighted and mean bags (sums not exact) and the forward with more than
512 slots: bounds derived in their tests' docstrings."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import sparse_optim_ref as ref  # noqa: E402
from oracle import tzrec_oracle as orc  # noqa: E402
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.embedding import EmbeddingBagCollection, EmbeddingBagConfig, SparseOptimizerConfig  # noqa: E402
from torcheasyrec_amd.sparse import KeyedJaggedTensor  # noqa: E402

DIMS = (4, 8, 12, 20, 24, 32, 48, 64, 128, 256)
EXACT = dict(rtol=2e-5, atol=1e-7)
U = 2.0 ** -24  # unit roundoff of fp32


def _sigma(B):
    """the scale of the dyadic gradients at batch B: the busiest rows of these tests sum up to ~B / 3 of them"""
    return 1.0 / 64 if B >= 1000 else 1.0 / 4


# (kind, weight_decay_mode): every optimizer of the library, row-wise Adagrad in its three weight-decay modes
ALL_KINDS = [("sgd", "none"), ("adagrad", "none"), ("rowwise_adagrad", "none"), ("rowwise_adagrad", "l2"),
             ("rowwise_adagrad", "decouple"), ("adam", "none")] + [(k, "none") for k in ref.NORM_KINDS]


def _cfg(kind, mode="none", **kw):
    wd = 0.0 if kind in ("sgd", "adagrad") or (kind == "rowwise_adagrad" and mode == "none") else 0.01
    a = dict(kind=kind, lr=0.5 if kind == "lars_sgd" else 0.02, beta1=0.8, beta2=0.95, weight_decay=wd, weight_decay_mode=mode,
             momentum=0.7)
    a.update(kw)
    return SparseOptimizerConfig(**a)


def _tables(spec, seed=0):
    """spec: (name, rows, D, pooling, key, data_type); weights uniform in [-0.1, 0.1)"""
    cfgs = []
    g = torch.Generator().manual_seed(seed)
    for name, rows, dim, pooling, key, dt in spec:
        w = (torch.rand(rows, dim, generator=g) - 0.5) * 0.2
        if dt == "FP16":
            w = w.half()
        cfgs.append(EmbeddingBagConfig(name, dim, rows, [key], pooling, init_fn=lambda t, w=w: t.copy_(w), data_type=dt))
    return cfgs


def _kjt(spec, B, rng, mode="uniform1", weighted=False, ids_fn=None):
    vals, lens = [], []
    for _, rows, _, _, _, _ in spec:
        L = np.ones(B, np.int32) if mode == "uniform1" else rng.poisson(2.0, size=B).astype(np.int32)
        if mode == "jagged":
            L[rng.integers(0, B, size=max(B // 8, 1))] = 0
        lens.append(L)
        n = int(L.sum())
        vals.append((ids_fn(rng, rows, n) if ids_fn else rng.integers(0, rows, size=n)).astype(np.int64))
    values = torch.from_numpy(np.concatenate(vals))
    w = torch.from_numpy(rng.uniform(0.5, 1.5, size=values.numel()).astype(np.float32)) if weighted else None
    return KeyedJaggedTensor([s[4] for s in spec], values, torch.from_numpy(np.concatenate(lens)), weights=w,
                             uniform_length=1 if mode == "uniform1" else None)


def _snapshot(ebc, kind):
    """{table: (weights, canonical state)} as numpy copies, read out of the storage in whatever layout it was allocated"""
    out = {}
    for t, c in enumerate(ebc.embedding_bag_configs()):
        st = ebc.table_states().get(c.name)
        store = ebc._storage[t].detach().cpu().numpy()
        w, m = ref.unpack(kind, c.embedding_dim, store, st.detach().cpu().numpy() if st is not None else None)
        out[c.name] = (w.copy(), None if m is None else m.copy())
    return out


def _lookup_grads(spec, kjt, up, B):
    """{table: (ids, dL/d(row contribution) per lookup)} of one KJT / upstream gradient"""
    off = orc.lengths_to_offsets(kjt.lengths().numpy())
    res, col = {}, 0
    for ki, (name, _, D, pooling, _, _) in enumerate(spec):
        s, e = off[ki * B], off[(ki + 1) * B]
        L = kjt.lengths().numpy()[ki * B:(ki + 1) * B]
        psw = kjt.weights_or_none().numpy()[s:e] if kjt.weights_or_none() is not None else None
        lg = orc.lookup_grads([up[:, col:col + D]], L, B, [pooling], psw)
        res[name] = (kjt.values().numpy()[s:e], lg)
        col += D
    return res


def _check_fp16(got, want, rows, msg):
    """test_fp16_tables' rule: one fp32 ulp of the update can flip the rounding to half -- within one half ulp, and all but a
    few elements of the touched rows exact (a share: counted where the touched rows hold 1000 elements or more)"""
    torch.testing.assert_close(torch.from_numpy(got.astype(np.float32)), torch.from_numpy(want.astype(np.float32)), rtol=1e-3,
                               atol=1e-5, msg=msg)
    if len(rows) * got.shape[1] >= 1000:
        assert float((got[rows] == want[rows]).mean()) > 0.98, msg


def _run_exact(dev, spec, cfg, B, steps=3, seed=3, ids_fn=None, row_layout="interleaved", hot=False, ebc_out=None, outs=None):
    """`steps` steps of one collection on one-id sum bags with dyadic upstream gradients.  The forward of each step is a copy
    of the looked-up rows (fp16: widened exactly): bit for bit against them.  After each step, weights and state of every
    table against one float64 update of the state the library held before it (EXACT; fp16 weights: the half-ulp rule).
    `outs`: a list that collects each step's output (cpu)."""
    rng = np.random.default_rng(seed)
    ebc = EmbeddingBagCollection(_tables(spec), device=dev, optimizer=cfg, row_layout=row_layout)
    ebc.expect_hot_rows = hot
    for step in range(steps):
        before = _snapshot(ebc, cfg.kind)
        kjt = _kjt(spec, B, rng, ids_fn=ids_fn)
        out = ebc(kjt.to(dev)).values()
        got_out = out.detach().cpu()
        gathered = [torch.from_numpy(before[name][0][kjt.values().numpy()[i * B:(i + 1) * B]].astype(np.float32))
                    for i, (name, *_) in enumerate(spec)]
        assert torch.equal(got_out, torch.cat(gathered, dim=1)), f"step {step}: the forward is not a copy of the rows"
        if outs is not None:
            outs.append(got_out)
        up = ref.dyadic_grads(rng, tuple(out.shape), _sigma(B))
        (out * torch.from_numpy(up).to(dev)).sum().backward()
        after = _snapshot(ebc, cfg.kind)
        for name, (ids, lg) in _lookup_grads(spec, kjt, up, B).items():
            ref.assert_exact_sums(ids, lg, _sigma(B))
            w, m = before[name]
            ref.sparse_update(w, m, ids, lg, cfg, step + 1, fp64=True)
            gw, gm = after[name]
            msg = f"step {step} {name} (D {w.shape[1]})"
            if w.dtype == np.float16:
                _check_fp16(gw, w, np.unique(ids), msg + " weights")
            else:
                np.testing.assert_allclose(gw, w, err_msg=msg + " weights", **EXACT)
            if m is not None:
                np.testing.assert_allclose(gm, m, err_msg=msg + " state", **EXACT)
    if ebc_out is not None:
        ebc_out.append(ebc)
    return ebc


# ---- mixed dims in one collection: max_dim = 256 beside D = 4 -------------------------------------------------------------
SPEC_MIXED = [(f"d{D}", rows, D, "sum", f"k{D}", "FP32")
              for D, rows in zip(DIMS, (300, 3, 50, 7, 120, 1000, 40, 5, 200, 60))]


@pytest.mark.parametrize("kind,mode", ALL_KINDS)
def test_mixed_dim_collection(dev, kind, mode, bwd_path):
    """one table per dim in one collection (3 to 1000 rows), one-id bags, 3 steps (Adam's bias correction moves)"""
    _run_exact(dev, SPEC_MIXED, _cfg(kind, mode), 64)
    assert (bwd_path["cells"] > 0, bwd_path["exact"] > 0) == (bwd_path["path"] == "cells", bwd_path["path"] == "planned")


@pytest.mark.parametrize("kind", ["sgd", "rowwise_adagrad", "adam", "lamb"])
def test_mixed_dim_collection_split_rows(dev, kind, bwd_path):
    """the same collection at B = 4000: the 3-, 5- and 7-row tables (D = 8, 48, 20) hold 570 - 1330 lookups a row -- split
    rows of the cells plan and row-split workgroups of the direct kernel, whose records and partial sums are laid out
    max_dim = 256 floats apart while the rows are narrower.  Pinned: the cells geometry of this batch plans partial-sum
    records (split rows); the direct kernel with only its row-split workgroups on (tzr_tune bwd_direct_debug = 5) still
    updates the 3-row table and leaves the 1000-row table alone"""
    B = 4000
    ebc = _run_exact(dev, SPEC_MIXED, _cfg(kind), B, steps=2)
    L = _lib.lib()
    if bwd_path["path"] == "cells":
        (meta,) = ebc._meta_cache.values()
        info = (C.c_int64 * 8)()
        _, max_dim = ebc._bwd_dims()
        assert L.tzr_bwd_cells_geometry(meta.bwd_tables_np.ctypes.data, len(SPEC_MIXED), meta.bwd_feats_np.ctypes.data,
                                        len(SPEC_MIXED), B, max_dim, None, 0, info) == 0
        assert info[5] > 0, "no split rows in the cells geometry"
    if bwd_path["path"] == "direct":
        probe = EmbeddingBagCollection(_tables(SPEC_MIXED), device=dev, optimizer=_cfg(kind))
        w0 = {n: w.detach().cpu().clone() for n, w in probe.table_weights().items()}
        kjt = _kjt(SPEC_MIXED, B, np.random.default_rng(5))
        assert L.tzr_tune(b"bwd_direct_debug", 5) == 0
        try:
            probe(kjt.to(dev)).values().sum().backward()
        finally:
            L.tzr_tune(b"bwd_direct_debug", 0)
        w1 = {n: w.detach().cpu() for n, w in probe.table_weights().items()}
        assert not torch.equal(w0["d8"], w1["d8"]), "the 3-row table went through no row-split workgroup"
        assert torch.equal(w0["d32"], w1["d32"])


# ---- hot rows at every dim ------------------------------------------------------------------------------------------------
def _half_on_one_row(rng, rows, n):
    ids = rng.integers(0, rows, size=n)
    ids[rng.random(n) < 0.5] = 4321 % rows
    return ids


HOT_CASES = [(D, k) for D in DIMS for k in ("sgd", "adagrad", "rowwise_adagrad", "adam")] + \
            [(D, k) for D in (8, 20, 128) for k in ref.NORM_KINDS]


@pytest.mark.parametrize("D,kind", HOT_CASES)
def test_hot_rows_per_dim(dev, D, kind, bwd_path):
    """a 5000-row table with half of its 3000 lookups on one row (more than an LDS unit holds: heavy tiles of the exact plan,
    split units of the cells plan, the hot row of the direct kernel) and a 3-row table (~1000 lookups a row: row-split
    workgroups of the direct kernel).  Adagrad and Adam tell the direct kernel to expect hot rows (TZR_GRAD_HOT_ROWS: every
    workgroup of the table takes a slice of the row), the others let the row's own range workgroup stream it."""
    spec = [("hot", 5000, D, "sum", "h", "FP32"), ("tiny", 3, D, "sum", "t", "FP32")]
    _run_exact(dev, spec, _cfg(kind), 3000, steps=2, ids_fn=_half_on_one_row, hot=kind in ("adagrad", "adam"))


# ---- layouts and dtypes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adagrad", "rowwise_adagrad"])
@pytest.mark.parametrize("D", DIMS)
def test_interleaved_and_split_layouts(dev, D, kind, bwd_path):
    """fp32 Adagrad / row-wise Adagrad with the state inside the weight row ([w | m], [w | m | pad]) and in an array of its
    own: each against the reference, and the two bit for bit alike (the same arithmetic on other addresses)"""
    spec = [("a", 700, D, "sum", "a", "FP32"), ("b", 9, D, "sum", "b", "FP32")]
    res = []
    for layout in ("interleaved", "split"):
        _run_exact(dev, spec, _cfg(kind, initial_accumulator_value=0.1), 96, steps=2, row_layout=layout, ebc_out=res)
    assert res[0]._storage[0].shape[1] == 2 * D and res[1]._storage[0].shape[1] == D
    for name in ("a", "b"):
        assert torch.equal(res[0].table_weights()[name].cpu(), res[1].table_weights()[name].cpu()), name
        assert torch.equal(res[0].table_states()[name].cpu(), res[1].table_states()[name].cpu()), name


@pytest.mark.parametrize("kind,mode", ALL_KINDS)
@pytest.mark.parametrize("D", [8, 12, 64, 256])
def test_fp16_tables_every_kind(dev, D, kind, mode, bwd_path):
    """`data_type: FP16` tables (half weights, fp32 state) beside an fp32 table of the same dim, every optimizer"""
    spec = [("h", 400, D, "sum", "h", "FP16"), ("f", 30, D, "sum", "f", "FP32"), ("h3", 3, D, "sum", "t", "FP16")]
    ebc = _run_exact(dev, spec, _cfg(kind, mode), 80, steps=2)
    assert ebc.table_weights()["h"].dtype == torch.float16


# ---- jagged, weighted and mean bags: sums that are not exact --------------------------------------------------------------
BOUND_KINDS = ("sgd", "adagrad", "rowwise_adagrad", "adam")


def _bounded_step_check(kind, cfg, step, w0, m0, ids, lg, gw, gm, msg):
    """One step from (w0, m0) with the lookup gradients lg (fp32 values as the kernel forms them) against float64, within a
    bound derived to first order.  The kernel's summed gradient of a row with n lookups differs from the exact sum by at most
    dg = (n + 1) u sum_i |g_i| (u = 2^-24: n - 1 additions in any order, and each g_i = upstream * weight / len carries up to
    two more roundings, already in lg -- the +1 covers them relative to the upstream values), the factor 2 below covering the
    second-order terms.  Through the update (m the new state, s = sqrt(v / c2)):
      sgd       dw = lr dg
      adagrad   dm = 2 |g| dg,                      dw = lr dg / sqrt(m) + lr |g| dm / (2 m^1.5)
      row-wise  dm = (2 / D) sum_d |g_d| dg_d,      dw = the same with the row's m
      adam      dm1 = (1 - b1) dg, dv = 2 (1 - b2) |g| dg,
                dw = lr ((1 - b1) dg / (c1 (s + eps)) + |m1 / c1| dv / (2 c2 s (s + eps)^2))
    plus the fp32 rounding of the update itself: 8 u (|w| + |w - w0|) on the weights, (D + 8) u |m| on the state (the row-wise
    mean is a sum of D squares).  The state starts non-zero (Adagrad 0.1, Adam exp_avg_sq 0.01): 1 / sqrt(m) stays bounded."""
    D = w0.shape[1]
    rows, g = ref.summed_rows64(ids, lg)
    _, ga = ref.summed_rows64(ids, np.abs(lg))
    _, n = np.unique(ids, return_counts=True)
    dg = 2 * (n[:, None] + 1) * U * ga
    w, m = w0.copy(), None if m0 is None else m0.copy()
    ref.update_rows(w, m, rows, g, cfg, step)
    lr, eps = float(np.float32(cfg.lr)), float(np.float32(cfg.eps))
    wr = w[rows].astype(np.float64)
    if kind == "sgd":
        dw = lr * dg
    elif kind in ("adagrad", "rowwise_adagrad"):
        mr = m[rows].astype(np.float64)
        if kind == "adagrad":
            dm = 2 * np.abs(g) * dg
        else:
            dm = (2.0 / D) * (np.abs(g) * dg).sum(axis=1)
            mr, dm = mr[:, None], dm[:, None]
        dw = lr * dg / np.sqrt(mr) + lr * np.abs(g) * dm / (2 * mr ** 1.5)
    else:
        b1, b2 = float(np.float32(cfg.beta1)), float(np.float32(cfg.beta2))
        c1, c2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        m1, v = m[rows, :D].astype(np.float64), m[rows, D:].astype(np.float64)
        s = np.sqrt(v / c2)
        dv = 2 * (1 - b2) * np.abs(g) * dg
        dw = lr * ((1 - b1) * dg / (c1 * (s + eps)) + np.abs(m1 / c1) * dv / (2 * c2 * s * (s + eps) ** 2))
        dm = np.concatenate([(1 - b1) * dg, dv], axis=1)
    bound_w = dw + 8 * U * (np.abs(wr) + np.abs(wr - w0[rows])) + 1e-12
    err_w = np.abs(gw[rows].astype(np.float64) - wr)
    assert (err_w <= bound_w).all(), f"{msg} weights: err {float((err_w - bound_w).max())} over the bound"
    others = np.setdiff1d(np.arange(w0.shape[0]), rows)
    assert np.array_equal(gw[others], w0[others]), msg + ": an untouched row moved"
    if m is not None:
        mr = m[rows].astype(np.float64)
        dm = dm.reshape(mr.shape) if kind == "rowwise_adagrad" else dm
        bound_m = dm + (D + 8) * U * np.abs(mr) + 1e-12
        err_m = np.abs(gm[rows].astype(np.float64) - mr)
        assert (err_m <= bound_m).all(), f"{msg} state: err {float((err_m - bound_m).max())} over the bound"


@pytest.mark.parametrize("kind", BOUND_KINDS)
@pytest.mark.parametrize("D", DIMS)
def test_jagged_weighted_and_mean_bags(dev, D, kind, bwd_path):
    """jagged bags (Poisson(2) ids, an eighth empty) with per-sample weights, one sum- and one mean-pooled table, 2 steps; the
    bound of _bounded_step_check on every touched element, untouched rows bit-identical"""
    spec = [("s", 400, D, "sum", "s", "FP32"), ("m", 25, D, "mean", "m", "FP32")]
    cfg = _cfg(kind, initial_accumulator_value=0.1, weight_decay=0.01 if kind == "adam" else 0.0)
    rng = np.random.default_rng(D)
    ebc = EmbeddingBagCollection(_tables(spec), device=dev, optimizer=cfg)
    for st in ebc.table_states().values():
        if kind == "rowwise_adagrad":
            st.fill_(0.1)
        elif kind == "adam":
            st[:, D:].fill_(0.01)
            st[:, :D].copy_(torch.from_numpy(rng.uniform(-0.01, 0.01, size=(st.shape[0], D)).astype(np.float32)))
    B = 48
    for step in range(2):
        before = _snapshot(ebc, kind)
        kjt = _kjt(spec, B, rng, mode="jagged", weighted=True)
        out = ebc(kjt.to(dev)).values()
        up = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        (out * torch.from_numpy(up).to(dev)).sum().backward()
        after = _snapshot(ebc, kind)
        for name, (ids, lg) in _lookup_grads(spec, kjt, up, B).items():
            w0, m0 = before[name]
            gw, gm = after[name]
            if len(ids):
                _bounded_step_check(kind, cfg, step + 1, w0, m0, ids, lg, gw, gm, f"step {step} {name} D {D}")


# ---- the forward that carries the plan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adagrad", "rowwise_adagrad", "adam"])
def test_forward_that_carries_the_plan_at_other_dims(dev, kind, monkeypatch):
    """tzr_pooled_fwd_cells_plan (forced at test sizes: fwd_plan = 2) with dims other than 16: 9 tables of D = 4 .. 128 (85
    slots), bit for bit against the two launches (outputs, weights, state), the outputs bit for bit against the looked-up rows
    and weights and state EXACT against the reference; a collection of 130 slots (> FWD1_SLOTS = 128) is declined and still
    right"""
    L = _lib.lib()
    monkeypatch.setenv("TZR_BWD_PLAN", "cells")
    assert L.tzr_tune(b"bwd_direct", -1) == 0 and L.tzr_tune(b"fwd_plan", 2) == 0
    try:
        cfg = _cfg(kind)
        spec = [(f"d{D}", rows, D, "sum", f"k{D}", "FP32")
                for D, rows in zip((4, 8, 12, 20, 24, 32, 48, 64, 128), (300, 3, 50, 7, 120, 1000, 40, 5, 200))]
        res, outs = [], {True: [], False: []}
        for carry in (True, False):
            made = []
            real = EmbeddingBagCollection.__init__

            def spy(self, *a, _real=real, **k):
                _real(self, *a, **k)
                self.forward_plan = carry
                made.append(self)

            monkeypatch.setattr(EmbeddingBagCollection, "__init__", spy)
            _run_exact(dev, spec, cfg, 200, steps=2, outs=outs[carry])
            monkeypatch.setattr(EmbeddingBagCollection, "__init__", real)
            assert made[0].forward_plans == (2 if carry else 0)
            res.append(made[0])
        assert len(outs[True]) == len(outs[False]) == 2
        for a, b in zip(outs[True], outs[False]):  # (each also a copy of the looked-up rows: _run_exact)
            assert torch.equal(a, b)
        for name in res[0].table_weights():
            assert torch.equal(res[0].table_weights()[name].cpu(), res[1].table_weights()[name].cpu()), name
            assert torch.equal(res[0].table_states()[name].cpu(), res[1].table_states()[name].cpu()), name
        wide = [("w0", 100, 256, "sum", "a", "FP32"), ("w1", 20, 256, "sum", "b", "FP32"), ("w2", 9, 8, "sum", "c", "FP32")]
        made = []
        real = EmbeddingBagCollection.__init__

        def spy2(self, *a, **k):
            real(self, *a, **k)
            made.append(self)

        monkeypatch.setattr(EmbeddingBagCollection, "__init__", spy2)
        _run_exact(dev, wide, cfg, 200, steps=2)
        assert made[0].forward_plans == 0
    finally:
        L.tzr_tune(b"bwd_direct", 0)
        L.tzr_tune(b"fwd_plan", 1)


# ---- the pooled forward with more than FWD_MAX_SLOTS = 512 slots ----------------------------------------------------------
@pytest.mark.parametrize("case", ["jagged", "weighted", "mean"])
def test_pooled_forward_over_512_slots(dev, case):
    """the general forward kernel splits the slots of a collection over blockIdx.y in rows of 512: 9 tables of D = 256 and
    one of D = 12 (579 slots: a second row of 67).  Table values and per-sample weights are dyadic (multiples of 2^-10 and
    2^-3 within +-1 and [0.5, 1.5]): products and sums are exact in fp32, so the sum and weighted cases must equal the
    float64 sums bit for bit.  A mean divides (or multiplies by 1 / len) once more: bound per element
    (n + 2) u sum_i |x_i| / len (any order of n - 1 additions, the scale and its product each rounding once), u = 2^-24."""
    rng = np.random.default_rng(7)
    spec = [(f"t{i}", 60 + i, 256, "mean" if case == "mean" else "sum", f"k{i}", "FP32") for i in range(9)]
    spec.append(("t12", 33, 12, "mean" if case == "mean" else "sum", "k12", "FP32"))
    inits = {s[0]: torch.from_numpy((rng.integers(-1024, 1024, size=(s[1], s[2])) / 1024.0).astype(np.float32)) for s in spec}
    cfgs = [EmbeddingBagConfig(n, D, rows, [k], p, init_fn=lambda t, w=inits[n]: t.copy_(w)) for n, rows, D, p, k, _ in spec]
    ebc = EmbeddingBagCollection(cfgs, device=dev)
    B = 37
    kjt = _kjt(spec, B, rng, mode="jagged")
    if case == "weighted":
        kjt = KeyedJaggedTensor(kjt.keys(), kjt.values(), kjt.lengths(),
                                weights=torch.from_numpy((rng.integers(4, 13, size=kjt.values().numel()) / 8.0).astype(np.float32)))
    assert sum(D // 4 for _, _, D, _, _, _ in spec) > 512
    got = ebc(kjt.to(dev)).values().detach().cpu().numpy().astype(np.float64)
    off = orc.lengths_to_offsets(kjt.lengths().numpy())
    psw = kjt.weights_or_none()
    col = 0
    for ki, (name, _, D, pooling, _, _) in enumerate(spec):
        tab = inits[name].numpy().astype(np.float64)
        for b in range(B):
            s, e = off[ki * B + b], off[ki * B + b + 1]
            terms = tab[kjt.values().numpy()[s:e]]
            if psw is not None:
                terms = terms * psw.numpy()[s:e, None].astype(np.float64)
            n = e - s
            scale = 1.0 / n if pooling == "mean" and n > 0 else 1.0
            want = terms.sum(axis=0) * scale
            bound = (n + 2) * U * np.abs(terms).sum(axis=0) * scale if pooling == "mean" else 0.0
            err = np.abs(got[b, col:col + D] - want)
            assert (err <= bound).all(), (name, b, float((err - bound).max()))
        col += D


# ---- the sequence EmbeddingCollection: one gradient row per id (grad_mode 1) ----------------------------------------------
@pytest.mark.parametrize("kind", ["adagrad", "adam"])
@pytest.mark.parametrize("D", [8, 32, 128, 256])
def test_sequence_collection(dev, D, kind, bwd_path):
    """unpooled lookups of two keys sharing one table plus a second table: every id's gradient row is its own (dyadic), the
    summed rows are exact -- 3 steps EXACT against the reference"""
    from torcheasyrec_amd.sequence import EmbeddingCollection, EmbeddingConfig

    rng = np.random.default_rng(D)
    g = torch.Generator().manual_seed(1)
    w0 = {"item_emb": (torch.rand(500, D, generator=g) - 0.5) * 0.2, "cat_emb": (torch.rand(4, D, generator=g) - 0.5) * 0.2}
    cfg = _cfg(kind)
    ec = EmbeddingCollection([EmbeddingConfig("item_emb", D, 500, ["item", "seq"], init_fn=lambda t: t.copy_(w0["item_emb"])),
                              EmbeddingConfig("cat_emb", D, 4, ["cat"], init_fn=lambda t: t.copy_(w0["cat_emb"]))],
                             device=dev, optimizer=cfg)
    keys, rows, B = ["item", "seq", "cat"], [500, 500, 4], 40
    for step in range(3):
        before = {n: (ec.table_weights()[n].detach().cpu().numpy().copy(), ec.table_states()[n].detach().cpu().numpy().copy())
                  for n in ("item_emb", "cat_emb")}
        lens = np.concatenate([np.ones(B, np.int32), rng.integers(0, 12, size=B).astype(np.int32), rng.integers(0, 4, size=B).astype(np.int32)])
        off = orc.lengths_to_offsets(lens)
        vals = np.concatenate([rng.integers(0, r, size=int(off[(i + 1) * B] - off[i * B])) for i, r in enumerate(rows)]).astype(np.int64)
        kjt = KeyedJaggedTensor(keys, torch.from_numpy(vals), torch.from_numpy(lens))
        jts = ec(kjt.to(dev))
        ups = {k: ref.dyadic_grads(rng, tuple(jts[k].values().shape), _sigma(B)) for k in keys}
        sum((jts[k].values() * torch.from_numpy(ups[k]).to(dev)).sum() for k in keys).backward()
        for name, ks in (("item_emb", ("item", "seq")), ("cat_emb", ("cat",))):
            ids = np.concatenate([vals[off[keys.index(k) * B]:off[(keys.index(k) + 1) * B]] for k in ks])
            lg = np.concatenate([ups[k] for k in ks], axis=0)
            ref.assert_exact_sums(ids, lg, _sigma(B))
            w, m = before[name]
            ref.sparse_update(w, m, ids, lg, cfg, step + 1, fp64=True)
            np.testing.assert_allclose(ec.table_weights()[name].detach().cpu().numpy(), w, err_msg=f"{name} weights", **EXACT)
            np.testing.assert_allclose(ec.table_states()[name].detach().cpu().numpy(), m, err_msg=f"{name} state", **EXACT)


# ---- production size on the GPU: the forms the library picks by itself ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dist", ["uniform", "zipf"])
def test_production_size_at_other_dims(dist, monkeypatch):
    """B = 65 536, three tables of 2 - 4 M rows at D = 8, 32, 128, Adagrad, no knobs: the library picks its forms.  Evenly drawn
    ids take the cells plan and the forward that carries it; Zipf ids overflow the cells' units in the probation batches and
    are demoted to the exact plan.  Two steps; the outputs bit for bit against the looked-up rows (a copy), weights and state
    of every touched row against a float64 reference built on
    the device, within the bound of test_fullsize_properties.test_adagrad_values_at_full_size (1e-5 relative, plus the fp32
    order-of-summation term eps32 sum |g_i| of rows that sum thousands of duplicates)."""
    from test_fullsize_properties import _row_sums
    from torcheasyrec_amd.criteo import SPARSE_KEYS, synthetic_batch

    monkeypatch.delenv("TZR_BWD_PLAN", raising=False)
    monkeypatch.delenv("TZR_FWD_PLAN", raising=False)
    _lib.use_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(17)
    rows, dims, B, lr, eps, eps32 = [4_000_000, 3_000_000, 2_000_000], [8, 32, 128], 65536, 0.05, 1e-8, 1.2e-7
    cfgs = [EmbeddingBagConfig(f"t{D}", D, r, [SPARSE_KEYS[i]]) for i, (r, D) in enumerate(zip(rows, dims))]
    ebc = EmbeddingBagCollection(cfgs, device=dev, optimizer=SparseOptimizerConfig(kind="adagrad", lr=lr, eps=eps,
                                                                                   initial_accumulator_value=0.1))
    for step in range(2):
        _, kjt, _ = synthetic_batch(60 + step, B, rows, dist=dist)
        kjt = kjt.to(dev)
        ids = kjt.values().view(len(rows), B)
        uniq, inv, w_before, m_before = [], [], [], []
        for f, c in enumerate(cfgs):
            u, i = torch.unique(ids[f], return_inverse=True)
            uniq.append(u)
            inv.append(i)
            w_before.append(ebc.table_weights()[c.name].detach()[u].double())
            m_before.append(ebc.table_states()[c.name].detach()[u].double())
        gathered = torch.cat([ebc.table_weights()[c.name].detach()[ids[f]] for f, c in enumerate(cfgs)], dim=1)
        out = ebc(kjt).values()
        assert torch.equal(out.detach(), gathered), f"step {step}: the forward is not a copy of the rows"
        del gathered
        g = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(200 + step)) * 0.1
        (out * g).sum().backward()
        torch.cuda.synchronize()
        col = 0
        for f, c in enumerate(cfgs):
            D = c.embedding_dim
            gf = g[:, col:col + D].double()
            col += D
            gs = _row_sums(inv[f], gf, uniq[f].numel())
            ga = _row_sums(inv[f], gf.abs(), uniq[f].numel())
            m_ref = m_before[f] + gs * gs
            w_ref = w_before[f] - lr * gs / (m_ref.sqrt() + eps)
            w_got = ebc.table_weights()[c.name].detach()[uniq[f]].double()
            m_got = ebc.table_states()[c.name].detach()[uniq[f]].double()
            w_err, m_err = (w_got - w_ref).abs(), (m_got - m_ref).abs()
            w_bound = 1e-5 * w_ref.abs() + 1e-9 + 4 * eps32 * lr * ga / m_ref.sqrt()
            m_bound = 1e-5 * m_ref.abs() + 8 * eps32 * ga * gs.abs()
            assert bool((w_err <= w_bound).all()), f"step {step} {c.name}: weight err {float((w_err - w_bound).max())} over the bound"
            assert bool((m_err <= m_bound).all()), f"step {step} {c.name}: state err {float((m_err - m_bound).max())} over the bound"
        del out
    if dist == "uniform":
        assert ebc.forward_plans == 2 and ebc.backward_form(kjt) == "cells"
    else:
        assert ebc.backward_form(kjt) == "exact"
