"""tests/golden/mind_mini.config through GraphTrainPipeline at B = 64, 12 sampled negatives, histories of 0 .. 23 clicks (every
batch the same lengths in another order: a replayed graph needs tensors of one shape): three eager steps followed by four steps
captured into / replayed from hipGraphs leave bit for bit what seven eager steps of an identically seeded twin leave -- the
capsule layer's and the attention's launches capture (argument structs are read when a launch is recorded, the offsets and the
upstream gradients from device memory; outputs, saved rows and the workspace are torch's buffers), the `normal` routing logits
are drawn on the device by torch's graph-safe generator, and every sum has a fixed order.  And the evaluation of the config's
recall@k, eager and replayed from a graph."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_mind_replays_from_a_graph():
    import mind_variants as mv
    from torcheasyrec_amd import _lib, capsule, match
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import GraphTrainPipeline
    from torcheasyrec_amd.match import ConfigMIND
    from torcheasyrec_amd.rank_model import build_rank_model

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(mv.TEXT)
    B, n_steps = 64, 7
    host = [b.pin_memory() for b in mv.batches(spec, B, n_steps, seed=9, fixed_total=True)]
    names = ("tzr_capsule_fwd", "tzr_capsule_bwd", "tzr_label_attn_fwd", "tzr_label_attn_bwd", "tzr_match_softmax_fwd")
    L = _lib.lib()
    orig, calls = {n: getattr(L, n) for n in names}, {n: 0 for n in names}
    for n in names:
        setattr(L, n, (lambda n: lambda *a: (calls.__setitem__(n, calls[n] + 1), orig[n](*a))[1])(n))
    res = []
    work = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(work):
            for graphs in (False, True):
                torch.manual_seed(3)
                model = build_rank_model(spec, device=dev)
                assert type(model) is ConfigMIND
                opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
                pipe = GraphTrainPipeline(model, opt, dev, model.loss, warmup=10 ** 9)  # (the twin never captures)
                it, losses = iter(host), []
                for step in range(n_steps):
                    if graphs and step == 3:
                        pipe._warmup = 0  # three eager steps lie behind: steps 3 and 4 capture their slot and replay, 5 and 6 replay
                    l, p, _ = pipe.progress(it)
                    assert sorted(l) == ["softmax_cross_entropy"] and sorted(p) == ["rank"]
                    losses.append(l["softmax_cross_entropy"].detach().clone())
                torch.cuda.synchronize()
                assert (pipe._graphs[0] is not None and pipe._graphs[1] is not None) == graphs  # captured without raising
                res.append((torch.stack(losses).cpu(),
                            {n: w.detach().cpu().clone() for n, w in model.state_dict().items() if ".embedding_group." in n},
                            {n: p.detach().cpu().clone() for n, p in model.named_parameters() if ".embedding_group." not in n}))
    finally:
        for n in names:
            setattr(L, n, orig[n])
    # the fused kernels are what ran: one call each per eager or captured step (7 eager steps, then 3 eager + 2 captured; replays
    # call nothing)
    assert capsule.FUSED_CAPSULE and match.FUSED_LABEL_ATTENTION and match.FUSED_MATCH_SOFTMAX
    assert calls == {n: 12 for n in names}
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la.tolist(), "eager then replayed", lb.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb) and float(la[0]) != float(la[-1])
    assert len(ta) == 6 and len(pa) == 18
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n


@pytest.mark.gpu
def test_mind_evaluates_recall_eager_and_from_a_graph():
    import mind_variants as mv
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.metrics import Evaluator, evaluate
    from torcheasyrec_amd.rank_model import build_rank_model

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(mv.TEXT.replace("num_iters: 3 }", 'num_iters: 3 routing_init_method: "zeros" }'))  # (no draw: the two runs see the same model)
    torch.manual_seed(4)
    model = build_rank_model(spec, device=dev)
    out = {}
    for graph in (False, True):
        host = [b.pin_memory() for b in mv.batches(spec, 64, 4, seed=10, fixed_total=True)]
        out[graph] = {k: float(v) for k, v in evaluate(model, host, Evaluator(model, spec, dev), graph=graph).items()}
        assert sorted(out[graph]) == ["recall@1", "recall@5"]
        assert 0.0 <= out[graph]["recall@1"] <= out[graph]["recall@5"] <= 1.0
    assert out[False] == out[True]  # (the same batches, the same counts)
