"""Adadelta and RMSprop on the MI355X: the graph-replayed training step and one step at full size on the DLRM-Criteo
tables."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_graph_pipeline_with_adadelta_matches_eager():
    """GraphTrainPipeline with Adadelta: 9 steps (2 eager warm-up steps, one capture per slot, then 5 replays) == 9 eager
    steps; the kind has no step counter, so nothing ticks inside the captured graph"""
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.criteo import CRITEO_ROWS, NUM_DENSE, SPARSE_KEYS, criteo_tables, synthetic_batch
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.dlrm import DLRM, bce_with_logits
    from torcheasyrec_amd.embedding import SparseOptimizerConfig
    from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch, GraphTrainPipeline, TrainPipeline
    from torcheasyrec_amd.sparse import KeyedTensor

    _lib.use_native()
    dev = torch.device("cuda", 0)
    rows = [min(r, 30000) for r in CRITEO_ROWS]
    B, n_steps = 1024, 9
    host = []
    for s in range(n_steps):
        d, k, l = synthetic_batch(s, B, rows, dist="zipf" if s % 2 else "uniform")
        host.append(Batch({BASE_DATA_GROUP: KeyedTensor([f"int_{i}" for i in range(NUM_DENSE)], [1] * NUM_DENSE, d)},
                          {BASE_DATA_GROUP: k}, {"label": l}).pin_memory())

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(5)
            self.m = DLRM(criteo_tables(rows, init="seeded"), SPARSE_KEYS, NUM_DENSE, device=dev,
                          sparse_optimizer=SparseOptimizerConfig(kind="adadelta", lr=1.0, rho=0.9, eps=1e-6,
                                                                 weight_decay=0.01))

        def forward(self, b):
            return self.m(b.dense_features[BASE_DATA_GROUP].values(), b.sparse_features[BASE_DATA_GROUP])

    loss_of = lambda pred, b: {"bce": bce_with_logits(pred, b.labels["label"])}  # noqa: E731
    res = []
    work = torch.cuda.Stream(dev)
    with torch.cuda.stream(work):
        for cls in (TrainPipeline, GraphTrainPipeline):
            model = M()
            opt = FusedDenseAdam(list(model.m.dense_parameters()), lr=1e-2)
            pipe = cls(model, opt, dev, loss_of)
            it = iter(host)
            losses = []
            while True:
                try:
                    l, _, _ = pipe.progress(it)
                except StopIteration:
                    break
                losses.append(float(l["bce"]))
            torch.cuda.synchronize()
            assert len(losses) == n_steps
            fo = model.m.ebc.fused_optimizer
            assert fo.cfg.kind == "adadelta" and fo._adam is None
            if cls is GraphTrainPipeline:
                assert pipe._graphs[0] is not None and pipe._graphs[1] is not None  # the late steps were replays
            res.append((losses, {n: w.detach().clone() for n, w in model.m.ebc.table_weights().items()},
                        {n: s.detach().clone() for n, s in model.m.ebc.table_states().items()}))
    (la, wa, sa), (lb, wb, sb) = res
    torch.testing.assert_close(torch.tensor(lb), torch.tensor(la), rtol=1e-6, atol=1e-7)
    for n in wa:
        torch.testing.assert_close(wb[n], wa[n], rtol=1e-5, atol=1e-6, msg=n)
        torch.testing.assert_close(sb[n], sa[n], rtol=1e-5, atol=1e-7, msg=n)
    assert all(float(s.abs().sum()) > 0.0 for s in sa.values())  # both running averages were written
    fresh = M()
    assert any(not torch.equal(wa[n], w.detach()) for n, w in fresh.m.ebc.table_weights().items())  # the tables moved


def test_rmsprop_at_full_size():
    """one step at B = 65 536 on the real 204 M-row tables with RMSprop: sampled touched rows (and a row nobody looked up)
    against an fp64 restatement built on the device from torch.unique + index_add_.

    Bound, per element: err = 2.4e-7 * (sum |g_i| + |wd w|), the fp32 order-of-summation bound of the summed gradient that
    test_partial_rowwise_adam_at_full_size uses (the small tables sum ~20 000 duplicates per row), carried through the
    formulas: the state s = (1 - alpha) g^2 moves by (1 - alpha)(2 |g| err + err^2); the step f(g) = g / (sqrt(s) + eps) is
    monotone in g, so it moves by at most max(f(g + err) - f(g), f(g) - f(g - err)) -- which is large where |g| is about err
    (the sign of a gradient that sums to nothing decides a whole step of lr / sqrt(1 - alpha): RMSprop's nature, not the
    kernel's).  On top, the project's fp32 tolerance for the arithmetic itself: 5e-5 relative + 1e-7."""
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.criteo import CRITEO_ROWS, SPARSE_KEYS, criteo_tables, synthetic_batch
    from torcheasyrec_amd.embedding import EmbeddingBagCollection, SparseOptimizerConfig

    _lib.use_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(13)
    B, D = 65536, 16
    lr, alpha, wd, eps = 0.002, 0.9, 0.01, 1e-8
    cfg = SparseOptimizerConfig(kind="rmsprop", lr=lr, alpha=alpha, eps=eps, weight_decay=wd)
    ebc = EmbeddingBagCollection(criteo_tables(CRITEO_ROWS), device=dev, optimizer=cfg, groups={"sparse": SPARSE_KEYS})
    _, kjt, _ = synthetic_batch(40, B, CRITEO_ROWS)
    kjt = kjt.to(dev)
    ids = kjt.values().view(26, B)
    g = torch.randn(B, 26 * D, device=dev, generator=torch.Generator(device=dev).manual_seed(100)) * 0.1
    rng = np.random.default_rng(0)
    picks = []
    for f, n in enumerate(ebc.table_weights()):
        u, inv = torch.unique(ids[f], return_inverse=True)
        sel = torch.from_numpy(rng.choice(u.numel(), size=min(64, u.numel()), replace=False)).to(dev)
        gf = g[:, f * D:(f + 1) * D].double()
        gs = torch.zeros(u.numel(), D, dtype=torch.float64, device=dev).index_add_(0, inv, gf)
        ga = torch.zeros(u.numel(), D, dtype=torch.float64, device=dev).index_add_(0, inv, gf.abs())
        w0 = ebc.table_weights()[n].detach()[u[sel]].double()
        untouched = None
        if u.numel() < CRITEO_ROWS[f]:
            mask = torch.ones(CRITEO_ROWS[f] if CRITEO_ROWS[f] < 1 << 20 else 1 << 20, dtype=torch.bool, device=dev)
            mask[u[u < mask.numel()]] = False
            free = torch.nonzero(mask)[:1, 0]
            if free.numel():
                untouched = (free, ebc.table_weights()[n].detach()[free].clone())
        picks.append((n, u[sel], gs[sel], ga[sel], w0, untouched))
    (ebc.forward_grouped(kjt)["sparse"] * g).sum().backward()
    torch.cuda.synchronize()
    c = (1 - alpha) ** 0.5

    def f_of(x):  # the first step's g / (sqrt(s) + eps) with s = (1 - alpha) g^2
        return x / (c * x.abs() + eps)

    checked = 0
    for n, rows, gs, ga, w0, untouched in picks:
        gg = gs + wd * w0
        err = 2.4e-7 * (ga + (wd * w0).abs())
        s = (1 - alpha) * gg * gg
        want = w0 - lr * f_of(gg)
        st = ebc.table_states()[n].detach()[rows].double()
        got_w = ebc.table_weights()[n].detach()[rows].double()
        assert st.shape == (rows.numel(), D)
        s_err = 5e-5 * s + (1 - alpha) * (2 * gg.abs() * err + err * err) + 1e-15
        print(f"{n}: state dev {float((st - s).abs().max()):.3e} weights dev {float((got_w - want).abs().max()):.3e}")
        assert bool(((st - s).abs() <= s_err).all()), (n, float((st - s).abs().max()))
        carry = torch.maximum(f_of(gg + err) - f_of(gg), f_of(gg) - f_of(gg - err))
        w_err = 5e-5 * want.abs() + 1e-7 + lr * carry
        assert bool(((got_w - want).abs() <= w_err).all()), (n, float(((got_w - want).abs() - w_err).max()))
        assert bool((got_w != w0).any())
        checked += rows.numel()
        if untouched is not None:
            assert torch.equal(ebc.table_weights()[n].detach()[untouched[0]], untouched[1]), n
            assert float(ebc.table_states()[n].detach()[untouched[0]].abs().sum()) == 0.0, n
    assert checked >= 26 * 3
