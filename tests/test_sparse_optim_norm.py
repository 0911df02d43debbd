"""The fused sparse optimizers of fbgemm's split TBE that came after Adam: partial row-wise Adam, LAMB, partial row-wise LAMB
and LARS-SGD (include/tzrec_hip.h at TZR_OPT_PARTIAL_ROWWISE_ADAM), from the tzrec config down to the row update of every
backward form, against the numpy restatement in tests/sparse_optim_ref.py."""
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
from torcheasyrec_amd.config import load_pipeline_spec, parse_text_proto, sparse_optimizer_from_config  # noqa: E402
from torcheasyrec_amd.embedding import EmbeddingBagCollection, EmbeddingBagConfig, SparseOptimizerConfig  # noqa: E402
from torcheasyrec_amd.sparse import KeyedJaggedTensor  # noqa: E402

KINDS = ref.NORM_KINDS


# ---- 1. config mapping -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,want", [
    ("partial_rowwise_adam_optimizer { lr: 0.01 beta1: 0.8 beta2: 0.95 weight_decay: 0.001 }",
     dict(kind="partial_rowwise_adam", lr=0.01, beta1=0.8, beta2=0.95, weight_decay=0.001)),
    ("lamb_optimizer { lr: 0.02 beta2: 0.9 }", dict(kind="lamb", lr=0.02, beta1=0.9, beta2=0.9, weight_decay=0.0)),
    ("partial_rowwise_lamb_optimizer { lr: 0.03 beta1: 0.7 weight_decay: 0.01 gradient_clipping: true max_gradient: 2.0 }",
     dict(kind="partial_rowwise_lamb", lr=0.03, beta1=0.7, beta2=0.999, weight_decay=0.01, gradient_clipping=True,
          max_gradient=2.0)),
    ("lars_sgd_optimizer { lr: 0.5 momentum: 0.8 weight_decay: 0.0001 }",
     dict(kind="lars_sgd", lr=0.5, momentum=0.8, weight_decay=0.0001, eta=0.001)),
    ("lars_sgd_optimizer { lr: 0.5 }", dict(kind="lars_sgd", lr=0.5, momentum=0.9)),
])
def test_config_maps_the_four_blocks(block, want):
    so = sparse_optimizer_from_config(parse_text_proto("sparse_optimizer { " + block + " }").one("sparse_optimizer"))
    for k, v in want.items():
        got = getattr(so, k)
        assert (got == v) if isinstance(v, (str, bool)) else abs(got - v) <= 1e-7 * max(1.0, abs(v)), (k, got, v)


# ---- 2. parity of every kind x backward form -------------------------------------------------------------------------------
def _tables(spec, seed=0, zero_rows=()):
    cfgs, inits = [], {}
    g = torch.Generator().manual_seed(seed)
    for name, rows, dim, pooling, key, dt in spec:
        w = (torch.rand(rows, dim, generator=g) - 0.5) * 0.2
        for r in zero_rows:
            if r < rows:
                w[r] = 0.0
        if dt == "FP16":
            w = w.half()
        inits[name] = w
        cfgs.append(EmbeddingBagConfig(name, dim, rows, [key], pooling, init_fn=lambda t, w=w: t.copy_(w), data_type=dt))
    return cfgs, inits


def _kjt(spec, B, rng, mode, weighted, ids_fn=None):
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


def _run(dev, spec, cfg, B, mode="uniform1", weighted=False, steps=3, seed=3, rtol=5e-5, zero_rows=(), grad_fn=None, ids_fn=None):
    """`steps` training steps of one EBC (one key per table); weights and state against the restatement after each run.
    grad_fn(rng, shape) -> the upstream gradient of the pooled output (default: standard normal)."""
    rng = np.random.default_rng(seed)
    cfgs, inits = _tables(spec, zero_rows=zero_rows)
    ebc = EmbeddingBagCollection(cfgs, device=dev, optimizer=cfg)
    w_ref = {n: inits[n].numpy().copy() for n in inits}
    m_ref = {n: np.zeros((w_ref[n].shape[0], ref.state_width(cfg.kind, w_ref[n].shape[1])), np.float32) for n in inits}
    for step in range(steps):
        kjt = _kjt(spec, B, rng, mode, weighted, ids_fn)
        out = ebc(kjt.to(dev)).values()
        up = grad_fn(rng, tuple(out.shape)) if grad_fn else rng.standard_normal(tuple(out.shape)).astype(np.float32)
        (out * torch.from_numpy(up).to(dev)).sum().backward()
        off = orc.lengths_to_offsets(kjt.lengths().numpy())
        col = 0
        for ki, (name, rows, D, pooling, key, _) in enumerate(spec):
            s, e = off[ki * B], off[(ki + 1) * B]
            L = kjt.lengths().numpy()[ki * B:(ki + 1) * B]
            psw = kjt.weights_or_none().numpy()[s:e] if weighted else None
            lg = orc.lookup_grads([up[:, col:col + D]], L, B, [pooling], psw)
            ref.sparse_update(w_ref[name], m_ref[name], kjt.values().numpy()[s:e], lg, cfg, step + 1)
            col += D
    for name, _, _, _, _, dt in spec:
        got = ebc.table_weights()[name].detach().cpu().float().numpy()
        want = w_ref[name].astype(np.float32)
        assert np.isfinite(got).all()
        if dt == "FP16":  # one half ulp apart at most where the fp32 results sit next to a rounding boundary
            np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-6, err_msg=f"weights of {name}")
        else:
            np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-7, err_msg=f"weights of {name}")
        st = ebc.table_states()[name].detach().cpu().numpy()
        assert st.shape == m_ref[name].shape
        np.testing.assert_allclose(st, m_ref[name], rtol=rtol, atol=1e-7, err_msg=f"state of {name}")
    return ebc


SPEC_SMALL = [("t_big", 5000, 16, "sum", "c0", "FP32"), ("t_mid", 300, 16, "sum", "c1", "FP32"),
              ("t_tiny", 3, 16, "sum", "c2", "FP32"), ("t_four", 4, 16, "sum", "c3", "FP32")]
# D = 4 (one lane per row), 12 (three lanes: a group that is not a power of two), 16, 64; one half-precision table; mean pooling
SPEC_DIMS = [("d4", 200, 4, "sum", "c0", "FP32"), ("d12", 150, 12, "mean", "c1", "FP32"), ("d16h", 100, 16, "sum", "c2", "FP16"),
             ("d64", 60, 64, "mean", "c3", "FP32")]


def _cfg(kind, wd=0.0, clip=False):
    return SparseOptimizerConfig(kind=kind, lr=0.02 if kind != "lars_sgd" else 0.5, beta1=0.8, beta2=0.95, weight_decay=wd,
                                 gradient_clipping=clip, max_gradient=0.9, momentum=0.7)


@pytest.mark.parametrize("kind", KINDS)
def test_uniform_one_id_bags(dev, kind, bwd_path):
    _run(dev, SPEC_SMALL, _cfg(kind), 64)
    assert (bwd_path["cells"] > 0, bwd_path["exact"] > 0) == (bwd_path["path"] == "cells", bwd_path["path"] == "planned")


@pytest.mark.parametrize("kind", KINDS)
def test_jagged_weighted_mean_clipped_decay_and_dims(dev, kind, bwd_path):
    _run(dev, SPEC_DIMS, _cfg(kind, wd=0.01, clip=True), 48, mode="jagged", weighted=True)


@pytest.mark.parametrize("kind", KINDS)
def test_long_runs(dev, kind, bwd_path):
    """1- and 3-row tables with thousands of lookups: rows split across units and combined by the last arriver (the
    whole-wave row update); fp32 order-of-summation noise over ~900-2600 gradients, so 5e-4 as the Adagrad case"""
    spec = [("t_one", 1, 16, "sum", "c0", "FP32"), ("t_tiny", 3, 16, "sum", "c1", "FP32")]
    _run(dev, spec, _cfg(kind), 2600, steps=2, rtol=5e-4)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_weight_row_and_zero_gradient_row(dev, kind, bwd_path):
    """row 0 of every table starts at zero (under the two LAMB kinds it does not move: r = 0); the upstream gradient is zero
    for half of the samples, so some touched rows have a summed gradient of exactly 0 (no NaN anywhere)"""
    def grad_fn(rng, shape):
        g = rng.standard_normal(shape).astype(np.float32)
        g[::2] = 0.0
        return g

    def ids_fn(rng, rows, n):  # row 0 looked up by sample 1 (a non-zero gradient) in every step
        ids = rng.integers(1, rows, size=n)
        ids[1] = 0
        return ids

    spec = [("a", 40, 16, "sum", "c0", "FP32"), ("b", 30, 12, "sum", "c1", "FP32")]
    ebc = _run(dev, spec, _cfg(kind), 32, zero_rows=(0,), grad_fn=grad_fn, ids_fn=ids_fn)
    if kind != "lars_sgd":  # (LARS: lambda = 0 for a zero row, its momentum stays 0)
        for n, st in ebc.table_states().items():
            assert float(st[0].abs().sum()) > 0.0, n  # row 0 was updated: its exp_avg moved
    if kind in ("lamb", "partial_rowwise_lamb"):
        for n, w in ebc.table_weights().items():
            assert float(w[0].abs().sum()) == 0.0, n


# ---- 3. partial row-wise Adam == Adam where every column of a row sees the same gradient ------------------------------------
def test_partial_rowwise_adam_equals_adam_on_column_constant_gradients(dev, bwd_path):
    def grad_fn(rng, shape):  # the same value in the 16 columns of each key's block, per sample
        g = rng.standard_normal((shape[0], shape[1] // 16)).astype(np.float32)
        return np.repeat(g, 16, axis=1)

    spec = [("t_big", 500, 16, "sum", "c0", "FP32"), ("t_tiny", 3, 16, "sum", "c1", "FP32")]
    res = {}
    for kind in ("adam", "partial_rowwise_adam"):
        rng = np.random.default_rng(7)
        cfgs, _ = _tables(spec)
        ebc = EmbeddingBagCollection(cfgs, device=dev, optimizer=SparseOptimizerConfig(kind=kind, lr=0.02, beta1=0.8,
                                                                                        beta2=0.95, weight_decay=0.01))
        for _ in range(3):
            kjt = _kjt(spec, 64, rng, "uniform1", False)
            out = ebc(kjt.to(dev)).values()
            (out * torch.from_numpy(grad_fn(rng, tuple(out.shape))).to(dev)).sum().backward()
        res[kind] = ebc
    for n in ("t_big", "t_tiny"):
        a, p = res["adam"], res["partial_rowwise_adam"]
        torch.testing.assert_close(p.table_weights()[n].cpu(), a.table_weights()[n].cpu(), rtol=2e-6, atol=1e-8)
        sa, sp = a.table_states()[n].cpu(), p.table_states()[n].cpu()
        torch.testing.assert_close(sp[:, :16], sa[:, :16], rtol=2e-6, atol=1e-9)  # exp_avg
        torch.testing.assert_close(sp[:, 16], sa[:, 16], rtol=2e-6, atol=1e-9)  # mean of g^2 == g_d^2


# ---- replicated tables: tzr_dense_rows_update{,_clear} ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clear", [0, 1])
def test_dense_rows_update(dev, kind, clear):
    """the all-reduced gradient rows of replicated tables (two tables in one concatenated row space, D = 12): rows with an
    all-zero gradient stay as they are"""
    rng = np.random.default_rng(11)
    D, rows = 12, [37, 20]
    cfg = _cfg(kind, wd=0.01)
    fo_ebc = EmbeddingBagCollection([EmbeddingBagConfig("x", D, 4, ["k"])], device=dev, optimizer=cfg)
    fo = fo_ebc.fused_optimizer
    ws = [torch.from_numpy((rng.random((r, D)) - 0.5).astype(np.float32)) for r in rows]
    ms = [torch.zeros(r, ref.state_width(kind, D)) for r in rows]
    ws_d, ms_d = [w.to(dev) for w in ws], [m.to(dev) for m in ms]
    tabs = np.zeros(2, dtype=_lib.TABLE_DT)
    for t in range(2):
        tabs[t]["w"], tabs[t]["m"], tabs[t]["rows"], tabs[t]["dim"] = _lib.ptr(ws_d[t]), _lib.ptr(ms_d[t]), rows[t], D
        tabs[t]["w_stride"], tabs[t]["m_stride"] = D, ms_d[t].stride(0)
    d_tabs = torch.from_numpy(tabs.view(np.uint8)).to(dev)
    start = torch.tensor([0, rows[0]], dtype=torch.int64, device=dev)
    wn, mn = [w.numpy().copy() for w in ws], [m.numpy().copy() for m in ms]
    for step in range(3):
        acc = rng.standard_normal((sum(rows), D)).astype(np.float32)
        acc[rng.random(sum(rows)) < 0.3] = 0.0
        acc_d = torch.from_numpy(acc.copy()).to(dev)
        fo.begin_step(dev)
        opt = fo.optim_struct(dev)
        f = _lib.lib().tzr_dense_rows_update_clear if clear else _lib.lib().tzr_dense_rows_update
        _lib.check(f(_lib.ptr(d_tabs), 2, _lib.ptr(start), sum(rows), _lib.ptr(acc_d), D, C.byref(opt), _lib.stream_ptr(dev)),
                   "dense_rows_update")
        for t in range(2):
            a = acc[(0 if t == 0 else rows[0]):(rows[0] if t == 0 else sum(rows))]
            nz = np.nonzero((a != 0).any(axis=1))[0]
            ref.update_rows(wn[t], mn[t], nz, a[nz], cfg, step + 1)
        if clear:
            assert float(acc_d.abs().sum()) == 0.0
    for t in range(2):
        np.testing.assert_allclose(ws_d[t].cpu().numpy(), wn[t], rtol=5e-5, atol=1e-7)
        np.testing.assert_allclose(ms_d[t].cpu().numpy(), mn[t], rtol=5e-5, atol=1e-7)


# ---- 5. checkpoint ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_config_trains_and_checkpoint_round_trips(dev, kind, tmp_path):
    """deepfm_mini.config with its sparse_optimizer swapped: parses, trains, and 2 steps + save + load into a fresh model +
    1 step == 3 uninterrupted steps, with the step counter restored"""
    from test_config_plumbing import _batches

    from torcheasyrec_amd.checkpoint import restore_checkpoint, save_checkpoint
    from torcheasyrec_amd.embedding_group import TrainPipeline
    from torcheasyrec_amd.rank_model import build_rank_model

    text = open(os.path.join(HERE, "golden", "deepfm_mini.config")).read()
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
    steps(a, batches)
    b = make()
    steps(b, batches[:2])
    save_checkpoint(str(tmp_path / "ck"), b)
    c = make()
    restore_checkpoint(str(tmp_path / "ck"), c)
    fo = c.embedding_group.ebc.fused_optimizer
    if kind != "lars_sgd":
        assert float(fo.adam_state(dev)[0]) == 2.0
    steps(c, batches[2:])
    if kind != "lars_sgd":
        assert float(fo.adam_state(dev)[0]) == 3.0
    for n, w in a.embedding_group.ebc.table_weights().items():
        assert torch.equal(w.detach(), c.embedding_group.ebc.table_weights()[n].detach()), n
    for n, s in a.embedding_group.ebc.table_states().items():
        assert torch.equal(s, c.embedding_group.ebc.table_states()[n]), n


# ---- 6. ABI argument checks ------------------------------------------------------------------------------------------------
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


def test_abi_accepts_the_new_kinds_and_refuses_a_missing_step_state(dev):
    L = _lib.lib()
    p = _lib.ptr
    tables, feats = torch.zeros(48, dtype=torch.uint8, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    vals, grad = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(64, device=dev)
    lr, st = torch.ones(1, device=dev), torch.zeros(4, device=dev)
    d = (_lib.TzrDst * 1)()
    d[0].ptr, d[0].stride = p(grad), 16
    start, acc = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(64, device=dev)
    # a cells geometry that passes its own checks (one chunk, one unit, this n_feats / max_dim): with no workspace, an
    # accepted kind stops at TZR_ERR_WORKSPACE, after the kind and d_adam checks
    h_geo = np.zeros(32, dtype=np.int64)
    h_geo[[0, 1, 4, 5]] = [1, 1, 1, 16]
    d_geo = _lib.workspace(256, dev)

    def optim(kind, with_step):
        o = _lib.TzrSparseOptim()
        o.kind, o.d_lr, o.eps, o.beta1, o.beta2 = kind, p(lr), 1e-8, 0.9, 0.999
        o.d_adam = p(st) if with_step else 0
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

    for kind in (_lib.OPT_PARTIAL_ROWWISE_ADAM, _lib.OPT_LAMB, _lib.OPT_PARTIAL_ROWWISE_LAMB):
        assert set(calls(optim(kind, False)).values()) == {INVALID}, kind  # no d_adam
    for kind in (_lib.OPT_PARTIAL_ROWWISE_ADAM, _lib.OPT_LAMB, _lib.OPT_PARTIAL_ROWWISE_LAMB, _lib.OPT_LARS_SGD):
        got = calls(optim(kind, kind != _lib.OPT_LARS_SGD or False))
        # accepted: each entry stops at its next check (no workspace / no cells geometry) or has nothing to do (0 rows)
        assert got == {"apply": WORKSPACE, "cells": WORKSPACE, "direct": WORKSPACE, "dense": OK, "dense_clear": OK}, (kind, got)
    assert set(calls(optim(9, True)).values()) == {UNSUPPORTED}
