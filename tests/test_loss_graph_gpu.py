"""tests/golden/jrc_mini.config (two-class output, jrc_loss over sessions, a sample weight column) through GraphTrainPipeline:
three eager steps followed by three steps replayed from the captured graphs leave bit for bit what six eager steps of an
identically seeded twin leave -- the sort of the session ids, the three launches of tzr_jrc_loss and the one-multiply backward
all capture, nothing reads the device -- and the Evaluator's `auc` reads `probs1`."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_jrc_loss_with_sample_weights_replays_from_a_graph():
    from examples.train_from_config import synthetic_batches
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import GraphTrainPipeline
    from torcheasyrec_amd.metrics import Evaluator, evaluate
    from torcheasyrec_amd.rank_model import build_rank_model

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(open(os.path.join(os.path.dirname(__file__), "golden", "jrc_mini.config")).read())
    B, n_steps = 256, 6
    host = [b.pin_memory() for b in synthetic_batches(spec, n_steps * B, B, seed=9)]
    res = []
    work = torch.cuda.Stream(dev)
    with torch.cuda.stream(work):
        for graphs in (False, True):
            torch.manual_seed(3)
            model = build_rank_model(spec, device=dev)
            opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
            pipe = GraphTrainPipeline(model, opt, dev, model.loss, warmup=10 ** 9)  # (the twin never captures)
            it, losses = iter(host), []
            for step in range(n_steps):
                if graphs and step == 3:
                    pipe._warmup = 0  # three eager steps lie behind: steps 3 and 4 capture their slot and replay, step 5 replays
                l, _, _ = pipe.progress(it)
                assert list(l) == ["jrc_loss"]
                losses.append(l["jrc_loss"].detach().clone())
            torch.cuda.synchronize()
            assert (pipe._graphs[0] is not None and pipe._graphs[1] is not None) == graphs  # captured without raising
            res.append((torch.stack(losses).cpu(), {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()},
                        [p.detach().cpu().clone() for p in model.dense_parameters()]))
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la.tolist(), "eager then replayed", lb.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    auc = evaluate(model, synthetic_batches(spec, 4 * B, B, seed=10), Evaluator(model, spec, dev))["auc"]
    print("auc", float(auc))
    assert 0.0 <= float(auc) <= 1.0
