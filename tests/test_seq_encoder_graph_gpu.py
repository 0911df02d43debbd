"""The mini config with a click history inside its DEEP group (tests/golden/mmoe_seq_mini.config) through GraphTrainPipeline:
the nested sequence group reaches its three encoders as jagged rows, so no step reads a length back from the device and the
whole step captures; three replays leave bit for bit what three eager steps of an identically seeded twin leave."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_sequence_encoders_in_a_deep_group_replay_from_a_graph():
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch, GraphTrainPipeline
    from torcheasyrec_amd.rank_model import build_rank_model
    from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(open(os.path.join(os.path.dirname(__file__), "golden", "mmoe_seq_mini.config")).read())
    B, n_steps, warmup = 64, 7, 2  # two slots: steps 0-3 warm up, 4 and 5 capture and replay, 6 replays
    rng = np.random.default_rng(8)
    sparse = [f for f in spec.features if f.is_sparse]
    dense = [f for f in spec.features if not f.is_sparse]
    base = rng.integers(0, 9, size=B).astype(np.int32)
    base[:2] = [0, 8]
    host = []
    for _ in range(n_steps):  # fixed-shape batches: every batch holds the same histories' lengths in another order
        ln_seq = rng.permutation(base)
        lens = [ln_seq if f.is_sequence else np.ones(B, np.int32) for f in sparse]
        vals = np.concatenate([rng.integers(0, f.num_embeddings, size=int(ln.sum())) for f, ln in zip(sparse, lens)]).astype(np.int64)
        ln = np.concatenate(lens)
        # (offsets made with the batch, on the host: a slot's cached offsets then travel with every batch copied into it)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(ln, dtype=np.int64)]))
        kjt = KeyedJaggedTensor([f.name for f in sparse], torch.from_numpy(vals), torch.from_numpy(ln), None, off)
        kt = KeyedTensor([f.name for f in dense], [f.value_dim for f in dense], torch.from_numpy(rng.random((B, len(dense)), dtype=np.float32)))
        host.append(Batch({BASE_DATA_GROUP: kt}, {BASE_DATA_GROUP: kjt},
                          {n: torch.from_numpy((rng.random(B) < 0.3).astype(np.int64)) for n in spec.label_fields}).pin_memory())
    res = []
    work = torch.cuda.Stream(dev)
    with torch.cuda.stream(work):
        for graphs in (False, True):
            torch.manual_seed(3)
            model = build_rank_model(spec, device=dev)
            assert model.embedding_group.jagged_sequence_groups == {"click_seq"}
            opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
            pipe = GraphTrainPipeline(model, opt, dev, model.loss, warmup=warmup if graphs else 10 ** 9)  # (the twin never captures)
            it, losses = iter(host), []
            for _ in range(n_steps):
                l, _, _ = pipe.progress(it)
                losses.append(torch.stack([l[k].detach() for k in sorted(l)]).clone())
            torch.cuda.synchronize()
            assert (pipe._graphs[0] is not None and pipe._graphs[1] is not None) == graphs  # captured without raising
            eg = model.embedding_group
            res.append((torch.stack(losses).cpu(), {n: w.detach().cpu().clone() for n, w in eg.ecs["16"].table_weights().items()},
                        [p.detach().cpu().clone() for p in model.dense_parameters()]))
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la[4:].tolist(), "replayed", lb[4:].tolist())
    assert torch.equal(la, lb)  # the three replays' losses included
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
