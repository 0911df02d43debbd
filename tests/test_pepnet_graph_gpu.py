"""tests/golden/pepnet_mini.config through GraphTrainPipeline at B = 64: three eager steps followed by four steps captured into /
replayed from hipGraphs leave bit for bit what seven eager steps of an identically seeded twin leave -- the gate-and-scale
launches of EPNet and of every PPNet level capture (the argument struct is read when the launch is recorded; outputs, gradients
and the partial-sum workspace are torch's buffers), the choice among a task's domain towers is a mask-and-sum that reads
nothing on the host, and the bias gradients are added in a fixed order."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_pepnet_replays_from_a_graph():
    from examples.train_from_config import synthetic_batches
    from torcheasyrec_amd import _lib, personalized_net
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import GraphTrainPipeline
    from torcheasyrec_amd.rank_model import ConfigPEPNet, build_rank_model

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(open(os.path.join(os.path.dirname(__file__), "golden", "pepnet_mini.config")).read())
    B, n_steps = 64, 7
    host = [b.pin_memory() for b in synthetic_batches(spec, n_steps * B, B, seed=9)]
    L = _lib.lib()
    orig, n_calls = L.tzr_gate_scale_fwd, [0]

    def counted(*a):
        n_calls[0] += 1
        return orig(*a)

    res = []
    work = torch.cuda.Stream(dev)
    L.tzr_gate_scale_fwd = counted
    try:
        with torch.cuda.stream(work):
            for graphs in (False, True):
                torch.manual_seed(3)
                model = build_rank_model(spec, device=dev)
                assert type(model) is ConfigPEPNet
                opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
                pipe = GraphTrainPipeline(model, opt, dev, model.loss, warmup=10 ** 9)  # (the twin never captures)
                it, losses = iter(host), []
                for step in range(n_steps):
                    if graphs and step == 3:
                        pipe._warmup = 0  # three eager steps lie behind: steps 3 and 4 capture their slot and replay, 5 and 6 replay
                    l, _, _ = pipe.progress(it)
                    assert sorted(l) == ["binary_cross_entropy_ctr", "binary_cross_entropy_cvr"]
                    losses.append(torch.stack([l["binary_cross_entropy_ctr"], l["binary_cross_entropy_cvr"]]).detach().clone())
                torch.cuda.synchronize()
                assert (pipe._graphs[0] is not None and pipe._graphs[1] is not None) == graphs  # captured without raising
                res.append((torch.stack(losses).cpu(), {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()},
                            {n: p.detach().cpu().clone() for n, p in model.named_parameters() if not n.startswith("embedding_group.")}))
    finally:
        L.tzr_gate_scale_fwd = orig
    # the fused step is what ran: EPNet and two PPNet levels per eager or captured step (7 eager steps, then 3 eager + 2 captured;
    # replays call nothing)
    assert personalized_net.FUSED_GATE_SCALE and n_calls[0] == (2 + 1) * 12
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la.tolist(), "eager then replayed", lb.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    assert len(pa) == 52
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
