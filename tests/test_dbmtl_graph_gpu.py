"""tests/golden/dbmtl_mini.config with its click history (tests/dbmtl_variants.py) through GraphTrainPipeline at B = 64: three eager steps followed by four steps captured into /
replayed from hipGraphs leave bit for bit what seven eager steps of an identically seeded twin leave -- the relation chain's
three launches capture (the argument struct is read when the launch is recorded; outputs, gradients and the workspace are
torch's buffers) and every sum of its backward has a fixed order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_dbmtl_replays_from_a_graph():
    from torcheasyrec_amd import _lib, rank_model
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch, GraphTrainPipeline
    from torcheasyrec_amd.rank_model import ConfigDBMTL, build_rank_model
    from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor

    _lib.use_native()
    dev = torch.device("cuda", 0)
    from dbmtl_variants import with_sequence

    spec = load_pipeline_spec(with_sequence())
    B, n_steps = 64, 7
    keys = ["binary_cross_entropy_ctr", "binary_cross_entropy_cvr", "binary_cross_entropy_pay"]
    rng = np.random.default_rng(9)
    sparse = [f for f in spec.features if f.is_sparse]
    dense = [f for f in spec.features if not f.is_sparse]
    base = rng.integers(0, 9, size=B).astype(np.int32)
    base[:2] = [0, 8]
    host = []
    for _ in range(n_steps):  # fixed-shape batches (tests/test_seq_encoder_graph_gpu.py): the same histories' lengths in another order
        ln_seq = rng.permutation(base)
        lens = [ln_seq if f.is_sequence else np.ones(B, np.int32) for f in sparse]
        vals = np.concatenate([rng.integers(0, f.num_embeddings, size=int(ln.sum())) for f, ln in zip(sparse, lens)]).astype(np.int64)
        ln = np.concatenate(lens)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(ln, dtype=np.int64)]))
        kjt = KeyedJaggedTensor([f.name for f in sparse], torch.from_numpy(vals), torch.from_numpy(ln), None, off)
        kt = KeyedTensor([f.name for f in dense], [f.value_dim for f in dense], torch.from_numpy(rng.random((B, len(dense)), dtype=np.float32)))
        host.append(Batch({BASE_DATA_GROUP: kt}, {BASE_DATA_GROUP: kjt},
                          {n: torch.from_numpy((rng.random(B) < 0.3).astype(np.int64)) for n in spec.label_fields}).pin_memory())
    L = _lib.lib()
    orig, n_calls = L.tzr_relation_chain_fwd, [0]

    def counted(*a):
        n_calls[0] += 1
        return orig(*a)

    res = []
    work = torch.cuda.Stream(dev)
    L.tzr_relation_chain_fwd = counted
    try:
        with torch.cuda.stream(work):
            for graphs in (False, True):
                torch.manual_seed(3)
                model = build_rank_model(spec, device=dev)
                assert type(model) is ConfigDBMTL
                opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
                pipe = GraphTrainPipeline(model, opt, dev, model.loss, warmup=10 ** 9)  # (the twin never captures)
                it, losses = iter(host), []
                for step in range(n_steps):
                    if graphs and step == 3:
                        pipe._warmup = 0  # three eager steps lie behind: steps 3 and 4 capture their slot and replay, 5 and 6 replay
                    l, _, _ = pipe.progress(it)
                    assert sorted(l) == keys
                    losses.append(torch.stack([l[k] for k in keys]).detach().clone())
                torch.cuda.synchronize()
                assert (pipe._graphs[0] is not None and pipe._graphs[1] is not None) == graphs  # captured without raising
                res.append((torch.stack(losses).cpu(), {f"{c}/{n}": w.detach().cpu().clone() for c, coll in [("ebc", model.embedding_group.ebc), ("ec", model.embedding_group.ecs["16"])]
                                                         for n, w in coll.table_weights().items()},
                            {n: p.detach().cpu().clone() for n, p in model.named_parameters()  # (dense_parameters(), by name)
                             if not n.startswith("embedding_group.") or n.startswith("embedding_group._group_name_to_seq_encoders.")}))
    finally:
        L.tzr_relation_chain_fwd = orig
    # the fused chain is what ran: one forward call per eager or captured step (7 eager steps, then 3 eager + 2 captured; replays
    # call nothing)
    assert rank_model.FUSED_RELATION_CHAIN and n_calls[0] == 12
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la.tolist(), "eager then replayed", lb.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    assert len(pa) >= 24
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
