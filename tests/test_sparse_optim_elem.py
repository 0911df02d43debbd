"""The two sparse optimizers without a step counter, Adadelta and RMSprop (include/tzrec_hip.h at TZR_OPT_ADADELTA), from
the tzrec config down to the row update of every backward form, against the numpy restatement in
tests/sparse_optim_elem_ref.py -- which test_restatement_is_torch pins to torch.optim.Adadelta / torch.optim.RMSprop.

Tolerances are the project's (tests/test_sparse_optim_norm.py): rtol 5e-5, atol 1e-7 for weights and state against the fp64
restatement, 5e-4 where thousands of gradients are summed in fp32, 1e-3 / 1e-6 for FP16 weights.  RMSprop's first steps are
about lr / sqrt(1 - alpha) in size whatever the gradient's scale, so its inputs here keep lr at the proto's default 0.002 with
alpha 0.9: the steps stay small against the weights.  Every parity run carries the SAME formula in fp32 numpy next to the
fp64 one and asserts that it passes the same tolerance first (reference against reference, no kernel involved): inputs on
which plain fp32 arithmetic could not meet the bound fail there, not at the kernel."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import sparse_optim_elem_ref as ref  # noqa: E402
from sparse_optim_ref import assert_exact_sums, dyadic_grads  # noqa: E402
from oracle import tzrec_oracle as orc  # noqa: E402
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.config import load_pipeline_spec, parse_text_proto, sparse_optimizer_from_config  # noqa: E402
from torcheasyrec_amd.embedding import EmbeddingBagCollection, EmbeddingBagConfig, SparseOptimizerConfig  # noqa: E402
from torcheasyrec_amd.sparse import KeyedJaggedTensor  # noqa: E402

KINDS = ref.ELEM_KINDS


# ---- 1. the restatement is torch's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 2.0 ** -7])
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_is_torch(kind, wd):
    """fp64, 6 steps, every row touched in every step (then lazy == dense): the restatement against torch.optim.Adadelta /
    torch.optim.RMSprop to 1e-12 relative.  The hyper-parameters are exact in fp32 (the restatement rounds them to fp32 as
    the C struct does), so both sides compute with the same numbers."""
    rng = np.random.default_rng(5)
    R, D = 50, 12
    lr, decay, eps = 2.0 ** -6, 0.875, 2.0 ** -20
    cfg = SparseOptimizerConfig(kind=kind, lr=lr, rho=decay, alpha=decay, eps=eps, weight_decay=wd)
    w = (rng.random((R, D)) - 0.5) * 0.2
    m = np.zeros((R, ref.state_width(kind, D)))
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = (torch.optim.Adadelta([p], lr=lr, rho=decay, eps=eps, weight_decay=wd) if kind == "adadelta"
           else torch.optim.RMSprop([p], lr=lr, alpha=decay, eps=eps, weight_decay=wd, momentum=0, centered=False))
    for _ in range(6):
        g = rng.standard_normal((R, D))
        ref.update_rows(w, m, np.arange(R), g, cfg)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=0)
    st = opt.state[p]
    np.testing.assert_allclose(m[:, :D], st["square_avg"].numpy(), rtol=1e-12, atol=0)
    if kind == "adadelta":
        np.testing.assert_allclose(m[:, D:], st["acc_delta"].numpy(), rtol=1e-12, atol=0)
    assert np.abs(m).max() > 0


# ---- 2. config mapping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,want", [
    ("adadelta_optimizer { lr: 0.5 rho: 0.9 eps: 1e-5 weight_decay: 0.001 gradient_clipping: true max_gradient: 2.0 }",
     dict(kind="adadelta", lr=0.5, rho=0.9, eps=1e-5, weight_decay=0.001, gradient_clipping=True, max_gradient=2.0)),
    ("adadelta_optimizer { }", dict(kind="adadelta", lr=0.002, rho=0.95, eps=1e-6, weight_decay=0.0, gradient_clipping=False,
                                    max_gradient=1.0)),
    ("rmsprop_optimizer { lr: 0.01 alpha: 0.9 eps: 1e-7 weight_decay: 0.01 gradient_clipping: true max_gradient: 0.5 }",
     dict(kind="rmsprop", lr=0.01, alpha=0.9, eps=1e-7, weight_decay=0.01, gradient_clipping=True, max_gradient=0.5)),
    ("rmsprop_optimizer { }", dict(kind="rmsprop", lr=0.002, alpha=0.99, eps=1e-8, weight_decay=0.0, gradient_clipping=False,
                                   max_gradient=1.0)),
])
def test_config_maps_the_two_blocks(block, want):
    so = sparse_optimizer_from_config(parse_text_proto("sparse_optimizer { " + block + " }").one("sparse_optimizer"))
    for k, v in want.items():
        got = getattr(so, k)
        assert (got == v) if isinstance(v, (str, bool)) else abs(got - v) <= 1e-7 * max(1.0, abs(v)), (k, got, v)


@pytest.mark.parametrize("kind", KINDS)
def test_config_refuses_eps_zero(kind):
    with pytest.raises(ValueError, match="eps"):
        sparse_optimizer_from_config(parse_text_proto("sparse_optimizer { %s_optimizer { eps: 0 } }" % kind).one("sparse_optimizer"))
    with pytest.raises(ValueError, match="eps"):  # ... and so does the collection, whoever built the config
        EmbeddingBagCollection([EmbeddingBagConfig("t", 8, 4, ["k"])], device=torch.device("cpu"),
                               optimizer=SparseOptimizerConfig(kind=kind, eps=0.0))


def test_the_other_kinds_keep_the_fixed_eps():
    for block in ("adagrad_optimizer { lr: 0.1 }", "adam_optimizer { }", "lamb_optimizer { }", "sgd_optimizer { }"):
        so = sparse_optimizer_from_config(parse_text_proto("sparse_optimizer { " + block + " }").one("sparse_optimizer"))
        assert so.eps == SparseOptimizerConfig().eps == 1e-8


# ---- 3. parity of both kinds x backward form --------------------------------------------------------------------------------
# spec rows: (table, rows, dim, pooling, [keys], data type); a table read by two keys gets the gradients of both
def _tables(spec, seed=0):
    cfgs, inits = [], {}
    g = torch.Generator().manual_seed(seed)
    for name, rows, dim, pooling, keys, dt in spec:
        w = (torch.rand(rows, dim, generator=g) - 0.5) * 0.2
        if dt == "FP16":
            w = w.half()
        inits[name] = w
        cfgs.append(EmbeddingBagConfig(name, dim, rows, list(keys), pooling, init_fn=lambda t, w=w: t.copy_(w), data_type=dt))
    return cfgs, inits


def _lookups(spec):
    """(table name, rows, dim, pooling, key) per lookup in the collection's own (table-major) order"""
    return [(name, rows, dim, pooling, k) for name, rows, dim, pooling, keys, _ in spec for k in keys]


def _kjt(spec, B, rng, mode, weighted, ids_fn=None):
    vals, lens, keys = [], [], []
    for _, rows, _, _, key in _lookups(spec):
        L = np.ones(B, np.int32) if mode == "uniform1" else rng.poisson(2.0, size=B).astype(np.int32)
        if mode == "jagged":
            L[rng.integers(0, B, size=max(B // 8, 1))] = 0
        lens.append(L)
        n = int(L.sum())
        vals.append((ids_fn(rng, rows, n) if ids_fn else rng.integers(0, rows, size=n)).astype(np.int64))
        keys.append(key)
    values = torch.from_numpy(np.concatenate(vals))
    w = torch.from_numpy(rng.uniform(0.5, 1.5, size=values.numel()).astype(np.float32)) if weighted else None
    return KeyedJaggedTensor(keys, values, torch.from_numpy(np.concatenate(lens)), weights=w,
                             uniform_length=1 if mode == "uniform1" else None)


def _check(got_w, got_m, w64, m64, name, dt, rtol, who):
    assert np.isfinite(got_w).all() and np.isfinite(got_m).all(), (who, name)
    if dt == "FP16":  # one half ulp apart at most where the fp32 results sit next to a rounding boundary
        np.testing.assert_allclose(got_w, w64.astype(np.float32), rtol=1e-3, atol=1e-6, err_msg=f"{who}: weights of {name}")
    else:
        np.testing.assert_allclose(got_w, w64, rtol=rtol, atol=1e-7, err_msg=f"{who}: weights of {name}")
    assert got_m.shape == m64.shape
    np.testing.assert_allclose(got_m, m64, rtol=rtol, atol=1e-7, err_msg=f"{who}: state of {name}")


def _run(dev, spec, cfg, B, mode="uniform1", weighted=False, steps=3, seed=3, rtol=5e-5, grad_fn=None, ids_fn=None, exact=False):
    """`steps` training steps of one EBC; weights and state against the restatement after the run.
    grad_fn(rng, shape) -> the upstream gradient of the pooled output (default: standard normal).  `exact`: the gradients
    are dyadic and every row's sum is checked to be exact in fp32 in any order; the restatement then sums in fp64."""
    rng = np.random.default_rng(seed)
    cfgs, inits = _tables(spec)
    ebc = EmbeddingBagCollection(cfgs, device=dev, optimizer=cfg)
    w64 = {n: inits[n].numpy().copy() for n in inits}  # updated in fp64, stored as the table's type
    w32 = {n: inits[n].numpy().copy() for n in inits}  # the same formula in fp32: reference against reference
    m64 = {n: np.zeros((w64[n].shape[0], ref.state_width(cfg.kind, w64[n].shape[1])), np.float32) for n in inits}
    m32 = {n: m64[n].copy() for n in inits}
    looks = _lookups(spec)
    for step in range(steps):
        kjt = _kjt(spec, B, rng, mode, weighted, ids_fn)
        out = ebc(kjt.to(dev)).values()
        up = grad_fn(rng, tuple(out.shape)) if grad_fn else rng.standard_normal(tuple(out.shape)).astype(np.float32)
        (out * torch.from_numpy(up).to(dev)).sum().backward()
        off = orc.lengths_to_offsets(kjt.lengths().numpy())
        per_table, col = {}, 0
        for ki, (name, rows, D, pooling, key) in enumerate(looks):
            s, e = off[ki * B], off[(ki + 1) * B]
            L = kjt.lengths().numpy()[ki * B:(ki + 1) * B]
            psw = kjt.weights_or_none().numpy()[s:e] if weighted else None
            lg = orc.lookup_grads([up[:, col:col + D]], L, B, [pooling], psw)
            per_table.setdefault(name, []).append((kjt.values().numpy()[s:e], lg))
            col += D
        for name, parts in per_table.items():
            ids, lg = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts], axis=0)
            if exact:
                assert_exact_sums(ids, lg)
            ref.sparse_update(w64[name], m64[name], ids, lg, cfg, fp64=exact)
            ref.sparse_update(w32[name], m32[name], ids, lg, cfg, fp64=exact, dtype=np.float32)
    for name, _, _, _, _, dt in spec:
        _check(w32[name].astype(np.float32), m32[name], w64[name], m64[name], name, dt, rtol, "fp32 restatement")
        _check(ebc.table_weights()[name].detach().cpu().float().numpy(), ebc.table_states()[name].detach().cpu().numpy(),
               w64[name], m64[name], name, dt, rtol, "kernel")
        assert np.abs(m64[name]).max() > 0 and not np.array_equal(w64[name], inits[name].numpy()), name  # the run trained
    return ebc


SPEC_SMALL = [("t_big", 5000, 16, "sum", ["c0"], "FP32"), ("t_mid", 300, 16, "sum", ["c1"], "FP32"),
              ("t_tiny", 3, 16, "sum", ["c2"], "FP32"), ("t_four", 4, 16, "sum", ["c3"], "FP32")]
# D = 8, 16 (half precision), 20 (five lanes: a group that is not a power of two), 64, 128; mean pooling; one table read by two keys
SPEC_DIMS = [("d8", 200, 8, "sum", ["c0"], "FP32"), ("d16h", 100, 16, "sum", ["c1"], "FP16"), ("d16", 90, 16, "mean", ["c2"], "FP32"),
             ("d20", 150, 20, "mean", ["c3", "c4"], "FP32"), ("d64", 60, 64, "mean", ["c5"], "FP32"),
             ("d128", 40, 128, "sum", ["c6"], "FP32")]


def _cfg(kind, wd=0.0, clip=False):
    if kind == "adadelta":
        return SparseOptimizerConfig(kind=kind, lr=0.5, rho=0.9, eps=1e-6, weight_decay=wd, gradient_clipping=clip, max_gradient=0.9)
    return SparseOptimizerConfig(kind=kind, lr=0.002, alpha=0.9, eps=1e-8, weight_decay=wd, gradient_clipping=clip, max_gradient=0.9)


@pytest.mark.parametrize("kind", KINDS)
def test_uniform_one_id_bags(dev, kind, bwd_path):
    _run(dev, SPEC_SMALL, _cfg(kind), 64)
    assert (bwd_path["cells"] > 0, bwd_path["exact"] > 0) == (bwd_path["path"] == "cells", bwd_path["path"] == "planned")
    assert (bwd_path["direct"] > 0) == (bwd_path["path"] == "direct")


@pytest.mark.parametrize("kind", KINDS)
def test_jagged_weighted_mean_clipped_decay_and_dims(dev, kind, bwd_path):
    """five steps: the running averages are read back non-zero four times"""
    _run(dev, SPEC_DIMS, _cfg(kind, wd=0.01, clip=True), 48, mode="jagged", weighted=True, steps=5)


@pytest.mark.parametrize("kind", KINDS)
def test_fp16_tables(dev, kind, bwd_path):
    spec = [("h16", 120, 16, "sum", ["c0"], "FP16"), ("h64", 50, 64, "sum", ["c1"], "FP16"), ("h8", 4, 8, "sum", ["c2"], "FP16")]
    _run(dev, spec, _cfg(kind, wd=0.01), 64, steps=4)


@pytest.mark.parametrize("kind", KINDS)
def test_long_runs(dev, kind, bwd_path):
    """1- and 3-row tables with thousands of lookups: rows split across units and combined by the last arriver (the
    whole-wave row update); fp32 order-of-summation noise over ~900-2600 gradients, so 5e-4 as the Adagrad case"""
    spec = [("t_one", 1, 16, "sum", ["c0"], "FP32"), ("t_tiny", 3, 16, "sum", ["c1"], "FP32")]
    _run(dev, spec, _cfg(kind), 2600, steps=3, rtol=5e-4)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_gradient_touched_row(dev, kind, bwd_path):
    """the upstream gradient is zero for every even sample and row 0 of each table is looked up by sample 0 alone: a touched row
    with a summed gradient of exactly 0 and no weight decay does not move (0 / eps-terms = 0) and nothing turns NaN; the rest
    of the run against the restatement as usual"""
    def grad_fn(rng, shape):
        g = rng.standard_normal(shape).astype(np.float32)
        g[::2] = 0.0
        return g

    def ids_fn(rng, rows, n):
        ids = rng.integers(1, rows, size=n)
        ids[0] = 0
        return ids

    spec = [("a", 40, 16, "sum", ["c0"], "FP32"), ("b", 30, 20, "sum", ["c1"], "FP32")]
    ebc = _run(dev, spec, _cfg(kind), 32, grad_fn=grad_fn, ids_fn=ids_fn)
    _, inits = _tables(spec)
    for n, w in ebc.table_weights().items():
        assert torch.equal(w.detach().cpu()[0], inits[n][0]), n
        assert float(ebc.table_states()[n][0].abs().sum()) == 0.0, n


@pytest.mark.parametrize("kind", KINDS)
def test_rows_nobody_looked_up_keep_weights_and_state(dev, kind, bwd_path):
    """two steps on rows [0, 100), then two on rows [100, 200): the first hundred rows -- state non-zero by then -- are the
    same bit for bit afterwards (no decay of the running averages of a row that is not looked up), weights and state"""
    spec = [("t", 200, 16, "sum", ["c0"], "FP32"), ("u", 200, 20, "sum", ["c1"], "FP32")]
    rng = np.random.default_rng(1)
    cfgs, _ = _tables(spec)
    ebc = EmbeddingBagCollection(cfgs, device=dev, optimizer=_cfg(kind, wd=0.01))

    def step(lo):
        kjt = _kjt(spec, 64, rng, "uniform1", False, ids_fn=lambda r, rows, n: r.integers(lo, lo + 100, size=n))
        out = ebc(kjt.to(dev)).values()
        (out * torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).to(dev)).sum().backward()

    step(0), step(0)
    snap = {n: (ebc.table_weights()[n].detach().cpu().clone(), ebc.table_states()[n].detach().cpu().clone()) for n in ("t", "u")}
    step(100), step(100)
    for n, (w, s) in snap.items():
        assert float(s[:100].abs().sum()) > 0.0 and float(s[100:].abs().sum()) == 0.0, n
        assert torch.equal(ebc.table_weights()[n].detach().cpu()[:100], w[:100]), n
        assert torch.equal(ebc.table_states()[n].detach().cpu()[:100], s[:100]), n
        assert float(ebc.table_states()[n].detach().cpu()[100:].abs().sum()) > 0.0, n


@contextlib.contextmanager
def _form(name, monkeypatch):
    """one backward form for the collections built inside, as the bwd_path fixture arranges it; yields the call counts"""
    L = _lib.lib()
    assert L.tzr_tune(b"bwd_direct", 1 if name == "direct" else -1) == 0
    monkeypatch.setenv("TZR_BWD_PLAN", "cells" if name == "cells" else "exact")
    names = {"direct": "tzr_pooled_bwd_direct", "cells": "tzr_pooled_bwd_cells_apply", "planned": "tzr_pooled_bwd_apply"}
    calls = {k: 0 for k in names}
    orig = {n: getattr(L, n) for n in names.values()}

    def counted(key):
        def f(*a):
            calls[key] += 1
            return orig[names[key]](*a)
        return f

    for k, n in names.items():
        setattr(L, n, counted(k))
    try:
        yield calls
    finally:
        for n, f in orig.items():
            setattr(L, n, f)
        L.tzr_tune(b"bwd_direct", 0)


@pytest.mark.parametrize("kind", KINDS)
def test_three_forms_agree_bit_for_bit(dev, kind, monkeypatch):
    """dyadic gradients: every row's summed gradient is exact in fp32 in any order (assert_exact_sums), so the planned, the
    cells and the direct kernel run the same row arithmetic on the same g -- and the row update spells every multiply-add as
    fmaf (csrc/pooled_bwd_apply.h: bwd_elem1), so the compiler's contraction has nothing to decide differently between the
    three instantiations: weights and state equal bit for bit after four steps with weight decay"""
    res = {}
    for form in ("planned", "cells", "direct"):
        with _form(form, monkeypatch) as calls:
            ebc = _run(dev, SPEC_SMALL, _cfg(kind, wd=0.01), 64, steps=4, grad_fn=lambda rng, shape: dyadic_grads(rng, shape), exact=True)
            assert [k for k, v in calls.items() if v > 0] == [form], (form, calls)
        res[form] = ({n: w.detach().cpu().clone() for n, w in ebc.table_weights().items()},
                     {n: s.detach().cpu().clone() for n, s in ebc.table_states().items()})
    for form in ("cells", "direct"):
        for n in res["planned"][0]:
            assert torch.equal(res[form][0][n], res["planned"][0][n]), (form, n, "weights")
            assert torch.equal(res[form][1][n], res["planned"][1][n]), (form, n, "state")


# ---- 4. replicated tables: tzr_dense_rows_update{,_clear}; the unpooled collection -----------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clear", [0, 1])
def test_dense_rows_update(dev, kind, clear):
    """the all-reduced gradient rows of replicated tables (two tables in one concatenated row space, D = 20): rows with an
    all-zero gradient stay as they are, weights and state"""
    rng = np.random.default_rng(11)
    D, rows = 20, [37, 20]
    cfg = _cfg(kind, wd=0.01)
    fo = EmbeddingBagCollection([EmbeddingBagConfig("x", D, 4, ["k"])], device=dev, optimizer=cfg).fused_optimizer
    ws = [torch.from_numpy(((rng.random((r, D)) - 0.5) * 0.2).astype(np.float32)) for r in rows]
    ms = [torch.zeros(r, ref.state_width(kind, D)) for r in rows]
    ws_d, ms_d = [w.to(dev) for w in ws], [m.to(dev) for m in ms]
    tabs = np.zeros(2, dtype=_lib.TABLE_DT)
    for t in range(2):
        tabs[t]["w"], tabs[t]["m"], tabs[t]["rows"], tabs[t]["dim"] = _lib.ptr(ws_d[t]), _lib.ptr(ms_d[t]), rows[t], D
        tabs[t]["w_stride"], tabs[t]["m_stride"] = D, ms_d[t].stride(0)
    d_tabs = torch.from_numpy(tabs.view(np.uint8)).to(dev)
    start = torch.tensor([0, rows[0]], dtype=torch.int64, device=dev)
    wn, mn = [w.numpy().copy() for w in ws], [m.numpy().copy() for m in ms]
    for step in range(4):
        acc = rng.standard_normal((sum(rows), D)).astype(np.float32)
        acc[rng.random(sum(rows)) < 0.3] = 0.0
        acc_d = torch.from_numpy(acc.copy()).to(dev)
        fo.begin_step(dev)
        opt = fo.optim_struct(dev)
        assert opt.d_adam == 0
        f = _lib.lib().tzr_dense_rows_update_clear if clear else _lib.lib().tzr_dense_rows_update
        _lib.check(f(_lib.ptr(d_tabs), 2, _lib.ptr(start), sum(rows), _lib.ptr(acc_d), D, C.byref(opt), _lib.stream_ptr(dev)),
                   "dense_rows_update")
        for t in range(2):
            a = acc[(0 if t == 0 else rows[0]):(rows[0] if t == 0 else sum(rows))]
            nz = np.nonzero((a != 0).any(axis=1))[0]
            ref.update_rows(wn[t], mn[t], nz, a[nz], cfg)
        if clear:
            assert float(acc_d.abs().sum()) == 0.0
    for t in range(2):
        np.testing.assert_allclose(ws_d[t].cpu().numpy(), wn[t], rtol=5e-5, atol=1e-7)
        np.testing.assert_allclose(ms_d[t].cpu().numpy(), mn[t], rtol=5e-5, atol=1e-7)
        assert np.abs(mn[t]).max() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_sequence_collection(dev, kind, bwd_path):
    """unpooled lookups of two keys sharing one table plus a second table: one gradient row per id (grad_mode 1), dyadic, so
    the summed rows are exact; 3 steps against the restatement"""
    from torcheasyrec_amd.sequence import EmbeddingCollection, EmbeddingConfig

    D, B = 32, 40
    rng = np.random.default_rng(D)
    g = torch.Generator().manual_seed(1)
    w0 = {"item_emb": (torch.rand(500, D, generator=g) - 0.5) * 0.2, "cat_emb": (torch.rand(4, D, generator=g) - 0.5) * 0.2}
    cfg = _cfg(kind, wd=0.01)
    ec = EmbeddingCollection([EmbeddingConfig("item_emb", D, 500, ["item", "seq"], init_fn=lambda t: t.copy_(w0["item_emb"])),
                              EmbeddingConfig("cat_emb", D, 4, ["cat"], init_fn=lambda t: t.copy_(w0["cat_emb"]))],
                             device=dev, optimizer=cfg)
    keys, rows = ["item", "seq", "cat"], [500, 500, 4]
    w = {n: w0[n].numpy().copy() for n in w0}
    m = {n: np.zeros((w[n].shape[0], ref.state_width(kind, D)), np.float32) for n in w0}
    for step in range(3):
        lens = np.concatenate([np.ones(B, np.int32), rng.integers(0, 12, size=B).astype(np.int32), rng.integers(0, 4, size=B).astype(np.int32)])
        off = orc.lengths_to_offsets(lens)
        vals = np.concatenate([rng.integers(0, r, size=int(off[(i + 1) * B] - off[i * B])) for i, r in enumerate(rows)]).astype(np.int64)
        kjt = KeyedJaggedTensor(keys, torch.from_numpy(vals), torch.from_numpy(lens))
        jts = ec(kjt.to(dev))
        ups = {k: dyadic_grads(rng, tuple(jts[k].values().shape)) for k in keys}
        sum((jts[k].values() * torch.from_numpy(ups[k]).to(dev)).sum() for k in keys).backward()
        for name, ks in (("item_emb", ("item", "seq")), ("cat_emb", ("cat",))):
            ids = np.concatenate([vals[off[keys.index(k) * B]:off[(keys.index(k) + 1) * B]] for k in ks])
            lg = np.concatenate([ups[k] for k in ks], axis=0)
            assert_exact_sums(ids, lg)
            ref.sparse_update(w[name], m[name], ids, lg, cfg, fp64=True)
    for name in w:
        np.testing.assert_allclose(ec.table_weights()[name].detach().cpu().numpy(), w[name], rtol=5e-5, atol=1e-7, err_msg=name)
        np.testing.assert_allclose(ec.table_states()[name].detach().cpu().numpy(), m[name], rtol=5e-5, atol=1e-7, err_msg=name)


# ---- 5. train from a config, checkpoint -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables_format", ["files", "dcp"])
@pytest.mark.parametrize("kind", KINDS)
def test_config_trains_and_checkpoint_round_trips(dev, kind, tables_format, tmp_path):
    """deepfm_mini.config with its sparse_optimizer swapped: parses, trains, and 2 steps + save + load into a fresh model +
    1 step == 3 uninterrupted steps; no step counter is written for these kinds"""
    from test_config_plumbing import _batches

    from torcheasyrec_amd.checkpoint import restore_checkpoint, save_checkpoint
    from torcheasyrec_amd.embedding_group import TrainPipeline
    from torcheasyrec_amd.rank_model import build_rank_model

    text = open(os.path.join(HERE, "golden", "deepfm_mini.config")).read()
    assert text.count("adagrad_optimizer") >= 1
    text = text.replace("adagrad_optimizer", f"{kind}_optimizer", 1)
    spec = load_pipeline_spec(text)
    assert spec.sparse_optimizer.kind == kind

    def make():
        torch.manual_seed(0)
        return build_rank_model(spec, device=dev)

    batches = list(_batches(spec, 3 * 16, 16, seed=1))

    def steps(model, bs):
        opt = torch.optim.SGD(list(model.dense_parameters()), lr=spec.dense_lr)
        pipe = TrainPipeline(model, opt, dev, model.loss)
        it = iter(bs)
        for _ in bs:
            pipe.progress(it)

    a = make()
    before = {n: w.detach().clone() for n, w in a.embedding_group.ebc.table_weights().items()}
    steps(a, batches)
    b = make()
    steps(b, batches[:2])
    save_checkpoint(str(tmp_path / "ck"), b, tables_format=tables_format)
    saved = torch.load(str(tmp_path / "ck" / "optimizer" / "rank0.pt"), weights_only=True)
    assert saved["adam_steps"] == {}
    c = make()
    restore_checkpoint(str(tmp_path / "ck"), c)
    for n, s in b.embedding_group.ebc.table_states().items():
        assert torch.equal(s, c.embedding_group.ebc.table_states()[n]) and float(s.abs().sum()) > 0.0, n
    steps(c, batches[2:])
    assert c.embedding_group.ebc.fused_optimizer._adam is None
    for n, w in a.embedding_group.ebc.table_weights().items():
        assert torch.equal(w.detach(), c.embedding_group.ebc.table_weights()[n].detach()), n
    for n, s in a.embedding_group.ebc.table_states().items():
        assert torch.equal(s, c.embedding_group.ebc.table_states()[n]), n
    assert any(not torch.equal(before[n], w.detach()) for n, w in a.embedding_group.ebc.table_weights().items())


# ---- 6. planner and byte model ----------------------------------------------------------------------------------------------
def test_planner_and_algorithmic_bytes_price_the_kinds():
    from torcheasyrec_amd.criteo import algorithmic_bytes
    from torcheasyrec_amd.planner import EmbeddingEnumerator, TableSpec, Topology

    en = EmbeddingEnumerator(Topology(2), 64)
    pairs = (("rmsprop", "adagrad"), ("adadelta", "adam"))
    for new, old in pairs:
        for bpe in (4, 2):
            a = en._state_bytes_dim(TableSpec("t", 1000, 16, optimizer=new, bytes_per_element=bpe, row_layout="split"), 1000, 16)
            b = en._state_bytes_dim(TableSpec("t", 1000, 16, optimizer=old, bytes_per_element=bpe, row_layout="split"), 1000, 16)
            assert a == b == 1000 * 16 * (4 if new == "rmsprop" else 8)
    ids = np.arange(8, dtype=np.int64) % 3
    base = algorithmic_bytes(ids, 4, [3, 3], 16, optimizer="sgd")
    U = base["U"]
    assert algorithmic_bytes(ids, 4, [3, 3], 16, optimizer="rmsprop")["bwd"] == algorithmic_bytes(ids, 4, [3, 3], 16, optimizer="adagrad")["bwd"]
    assert algorithmic_bytes(ids, 4, [3, 3], 16, optimizer="rmsprop")["bwd"] - base["bwd"] == 8 * 16 * U
    assert algorithmic_bytes(ids, 4, [3, 3], 16, optimizer="adadelta")["bwd"] - base["bwd"] == 16 * 16 * U


# ---- 7. ABI argument checks -------------------------------------------------------------------------------------------------
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


def test_abi_accepts_kinds_9_and_10_without_a_step_state(dev):
    """every backward entry point takes TZR_OPT_ADADELTA / TZR_OPT_RMSPROP with d_adam = 0 (each call then stops at its next
    check: no workspace, or nothing to do for 0 rows); eps <= 0 is an invalid argument for these two kinds, a step state
    an unsupported request; a kind nobody knows is still a status code"""
    L = _lib.lib()
    p = _lib.ptr
    assert (_lib.OPT_ADADELTA, _lib.OPT_RMSPROP) == (9, 10)
    tables, feats = torch.zeros(48, dtype=torch.uint8, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    vals, grad = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(64, device=dev)
    lr = torch.ones(1, device=dev)
    d = (_lib.TzrDst * 1)()
    d[0].ptr, d[0].stride = p(grad), 16
    start, acc = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(64, device=dev)
    h_geo = np.zeros(32, dtype=np.int64)
    h_geo[[0, 1, 4, 5]] = [1, 1, 1, 16]
    d_geo = _lib.workspace(256, dev)

    step_state = torch.zeros(4, device=dev)

    def optim(kind, eps=1e-6, with_step=False):
        o = _lib.TzrSparseOptim()
        o.kind, o.d_lr, o.eps, o.beta1, o.beta2, o.d_adam = kind, p(lr), eps, 0.9, 0.0, p(step_state) if with_step else 0
        return o

    def calls(o):
        r = C.byref(o)
        return {
            "apply": L.tzr_pooled_bwd_apply(p(tables), p(feats), 1, 1, 16, None, None, 4, 4, 4, 1, 0, d, 1, r, None, 0, None),
            "cells": L.tzr_pooled_bwd_cells_apply(p(tables), p(feats), 1, 1, 16, None, 4, 4, 0, d, 1, r, h_geo.ctypes.data, p(d_geo),
                                                  None, 0, None),
            "direct": L.tzr_pooled_bwd_direct(p(tables), 1, p(feats), 1, 10, 16, p(vals), None, None, 4, 4, 4, 1, 0, d, 1, r,
                                              None, 0, None),
            "dense": L.tzr_dense_rows_update(p(tables), 1, p(start), 0, p(acc), 16, r, None),
            "dense_clear": L.tzr_dense_rows_update_clear(p(tables), 1, p(start), 0, p(acc), 16, r, None),
        }

    for kind in (_lib.OPT_ADADELTA, _lib.OPT_RMSPROP):
        got = calls(optim(kind))
        assert got == {"apply": WORKSPACE, "cells": WORKSPACE, "direct": WORKSPACE, "dense": OK, "dense_clear": OK}, (kind, got)
        assert set(calls(optim(kind, eps=0.0)).values()) == {INVALID}, kind
        assert set(calls(optim(kind, eps=-1e-6)).values()) == {INVALID}, kind
        # neither kind has a step: a step state asks for a variant this build has no kernel for (include/tzrec_hip.h)
        assert set(calls(optim(kind, with_step=True)).values()) == {UNSUPPORTED}, kind
    for kind in (11, 12, 99, -1):
        assert set(calls(optim(kind)).values()) == {UNSUPPORTED}, kind


@pytest.mark.parametrize("kind", KINDS)
def test_state_stride_is_checked(kind):
    from torcheasyrec_amd.embedding import check_state_stride

    D = 16
    need = ref.state_width(kind, D)
    check_state_stride(kind, D, need)
    check_state_stride(kind, D, need + 4)
    with pytest.raises(ValueError, match="stride"):
        check_state_stride(kind, D, need - 4)
