"""tests/golden/rocket_mini.config and two variants (tests/rocket_variants.py) through GraphTrainPipeline at B = 64: three eager steps
followed by four steps captured into / replayed from hipGraphs leave bit for bit what seven eager steps of an identically seeded
twin leave -- the distillation launches capture (the argument struct is read when the launch is recorded, the upstream gradients
from device memory; outputs, the saved scale and the workspace are torch's buffers), the light net reads a detached share MLP, and
every sum has a fixed order.  And the evaluation of the config's auc -- `auc_light` -- eager and replayed from a graph."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

VARIANTS = ["mini", "two_class", "distance"]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_rocket_launching_replays_from_a_graph(variant):
    import rocket_variants as rv
    from torcheasyrec_amd import _lib, rocket
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import GraphTrainPipeline
    from torcheasyrec_amd.rank_model import build_rank_model
    from torcheasyrec_amd.rocket import ConfigRocketLaunching

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(rv.variant(variant))
    B, n_steps = 64, 7
    host = [b.pin_memory() for b in rv.batches(spec, B, n_steps, seed=9)]
    kind = "softmax_cross_entropy" if variant == "two_class" else "binary_cross_entropy"
    loss_keys = sorted([kind + "_booster", kind + "_light", "hint_l2_loss", "similarity_0_1", "similarity_1_2"])
    L = _lib.lib()
    orig, n_calls = L.tzr_distill_loss_fwd, [0]

    def counted(*a):
        n_calls[0] += 1
        return orig(*a)

    res = []
    work = torch.cuda.Stream(dev)
    L.tzr_distill_loss_fwd = counted
    try:
        with torch.cuda.stream(work):
            for graphs in (False, True):
                torch.manual_seed(3)
                model = build_rank_model(spec, device=dev)
                assert type(model) is ConfigRocketLaunching
                opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
                pipe = GraphTrainPipeline(model, opt, dev, model.loss, warmup=10 ** 9)  # (the twin never captures)
                it, losses = iter(host), []
                for step in range(n_steps):
                    if graphs and step == 3:
                        pipe._warmup = 0  # three eager steps lie behind: steps 3 and 4 capture their slot and replay, 5 and 6 replay
                    l, p, _ = pipe.progress(it)
                    assert sorted(l) == loss_keys and "logits_light" in p and "logits_booster" in p
                    losses.append(torch.stack([l[k].detach() for k in loss_keys]).clone())
                torch.cuda.synchronize()
                assert (pipe._graphs[0] is not None and pipe._graphs[1] is not None) == graphs  # captured without raising
                res.append((torch.stack(losses).cpu(),
                            {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()},
                            {n: p.detach().cpu().clone() for n, p in model.named_parameters() if not n.startswith("embedding_group.")}))
    finally:
        L.tzr_distill_loss_fwd = orig
    # the fused terms are what ran: one forward call per eager or captured step (7 eager steps, then 3 eager + 2 captured; replays
    # call nothing)
    assert rocket.FUSED_DISTILL_LOSS and n_calls[0] == 12
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la.tolist(), "eager then replayed", lb.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb) and not torch.equal(la[0], la[-1])
    assert len(ta) == 3 and len(pa) == 16
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["mini", "two_class"])
def test_rocket_launching_evaluates_auc_light_eager_and_from_a_graph(variant):
    import rocket_variants as rv
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.metrics import Evaluator, evaluate
    from torcheasyrec_amd.rank_model import build_rank_model

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(rv.variant(variant))
    torch.manual_seed(4)
    model = build_rank_model(spec, device=dev)
    out = {}
    for graph in (False, True):
        host = [b.pin_memory() for b in rv.batches(spec, 64, 4, seed=10)]
        out[graph] = {k: float(v) for k, v in evaluate(model, host, Evaluator(model, spec, dev), graph=graph).items()}
        assert sorted(out[graph]) == ["auc_light"] and 0.0 <= out[graph]["auc_light"] <= 1.0
    assert out[False] == out[True]  # (the same batches, the same counts)
