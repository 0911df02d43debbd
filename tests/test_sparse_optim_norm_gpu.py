"""The norm-based and partial row-wise sparse optimizers on the MI355X: the graph-replayed training step (the device step
counter ticks inside the captured graph) and one step at full size on the DLRM-Criteo tables."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_graph_pipeline_with_lamb_matches_eager():
    """GraphTrainPipeline with LAMB: 9 steps (2 eager warm-up steps, one capture per slot, then 5 replays) == 9 eager steps,
    and the step counter reached 9 both ways (the tick is one of the captured launches)"""
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
                          sparse_optimizer=SparseOptimizerConfig(kind="lamb", lr=0.05, beta1=0.8, beta2=0.95,
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
            assert float(fo.adam_state(dev)[0]) == n_steps
            if cls is GraphTrainPipeline:
                assert pipe._graphs[0] is not None and pipe._graphs[1] is not None  # the late steps were replays
            res.append((losses, {n: w.detach().clone() for n, w in model.m.ebc.table_weights().items()},
                        {n: s.detach().clone() for n, s in model.m.ebc.table_states().items()}))
    (la, wa, sa), (lb, wb, sb) = res
    torch.testing.assert_close(torch.tensor(lb), torch.tensor(la), rtol=1e-6, atol=1e-7)
    for n in wa:
        torch.testing.assert_close(wb[n], wa[n], rtol=1e-5, atol=1e-6, msg=n)
        torch.testing.assert_close(sb[n], sa[n], rtol=1e-5, atol=1e-7, msg=n)
    fresh = M()
    assert any(not torch.equal(wa[n], w.detach()) for n, w in fresh.m.ebc.table_weights().items())  # the tables moved


def test_partial_rowwise_adam_at_full_size():
    """one step at B = 65 536 on the real 204 M-row tables with partial row-wise Adam: sampled touched rows (and a row nobody
    looked up) against an fp64 restatement built on the device from torch.unique + segmented sums"""
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.criteo import CRITEO_ROWS, SPARSE_KEYS, criteo_tables, synthetic_batch
    from torcheasyrec_amd.embedding import EmbeddingBagCollection, SparseOptimizerConfig

    _lib.use_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(13)
    B, D = 65536, 16
    cfg = SparseOptimizerConfig(kind="partial_rowwise_adam", lr=0.01, beta1=0.8, beta2=0.95, weight_decay=0.01)
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
        picks.append((n, u[sel], gs[sel], 2.4e-7 * ga[sel], w0, untouched))
    (ebc.forward_grouped(kjt)["sparse"] * g).sum().backward()
    torch.cuda.synchronize()
    b1, b2, lr, wd, eps = 0.8, 0.95, 0.01, 0.01, 1e-8
    c1, c2 = 1 - b1, 1 - b2
    for n, rows, gs, err, w0, untouched in picks:
        # err = the fp32 order-of-summation bound of the summed gradient (eps32 * sum |g_i|: the small tables sum ~20 000
        # duplicates per row), carried through each formula
        m = (1 - b1) * gs
        v = (1 - b2) * (gs * gs).mean(dim=1, keepdim=True)
        want = w0 - lr * ((m / c1) / (torch.sqrt(v / c2) + eps) + wd * w0)
        st = ebc.table_states()[n].detach()[rows].double()
        got_w = ebc.table_weights()[n].detach()[rows].double()
        rms = torch.sqrt((gs * gs).mean(dim=1, keepdim=True)) + 1e-30
        assert bool(((st[:, :D] - m).abs() <= 1e-5 * m.abs() + (1 - b1) * err + 1e-12).all()), n
        v_err = (1 - b2) * (2 * gs.abs() * err + err * err).mean(dim=1, keepdim=True)
        assert bool(((st[:, D:D + 1] - v).abs() <= 2e-5 * v + v_err + 1e-15).all()), n
        w_err = 2e-5 * want.abs() + 1e-6 + lr * 3 * err / rms  # (u = gs / rms(gs) at the first step)
        assert bool(((got_w - want).abs() <= w_err).all()), (n, float((got_w - want).abs().max()))
        if untouched is not None:
            assert torch.equal(ebc.table_weights()[n].detach()[untouched[0]], untouched[1]), n
