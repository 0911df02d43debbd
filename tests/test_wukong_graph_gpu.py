"""tests/golden/wukong_mini.config through GraphTrainPipeline at B = 64: three eager steps followed by four steps captured into /
replayed from hipGraphs leave bit for bit what seven eager steps of an identically seeded twin leave -- each layer's two launches
of the forward, the backward's two pairs (the pass over the batch and its fixed-order finish) and the workspaces they take from
the allocator all capture (every pointer travels by value; the tensors keep their addresses), nothing reads the device.  The
LayerNorm parameters are perturbed first: weight 1 and bias 0 would hide them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

ENTRY_POINTS = ("tzr_wukong_fm_fwd", "tzr_wukong_mix_fwd", "tzr_wukong_fm_bwd", "tzr_wukong_mix_bwd")


@pytest.mark.gpu
def test_wukong_replays_from_a_graph():
    from examples.train_from_config import synthetic_batches
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import GraphTrainPipeline
    from torcheasyrec_amd.rank_model import ConfigWuKong, build_rank_model

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(open(os.path.join(os.path.dirname(__file__), "golden", "wukong_mini.config")).read())
    B, n_steps = 64, 7
    host = [b.pin_memory() for b in synthetic_batches(spec, n_steps * B, B, seed=9)]
    lib, calls = _lib.lib(), [0, 0]
    orig = {nm: getattr(lib, nm) for nm in ENTRY_POINTS}

    def counted(nm, slot):
        def f(*a):
            calls[slot] += 1
            return orig[nm](*a)
        return f

    for i, nm in enumerate(ENTRY_POINTS):
        setattr(lib, nm, counted(nm, i // 2))
    res = []
    work = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(work):
            for graphs in (False, True):
                torch.manual_seed(3)
                model = build_rank_model(spec, device=dev)
                assert type(model) is ConfigWuKong and len(model._wukong_layers) == 2
                with torch.no_grad():
                    for m in model.modules():
                        if isinstance(m, torch.nn.LayerNorm):
                            m.weight.copy_((1.0 + 0.3 * torch.randn(m.weight.shape)).to(dev))
                            m.bias.copy_((0.3 * torch.randn(m.bias.shape)).to(dev))
                opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
                pipe = GraphTrainPipeline(model, opt, dev, model.loss, warmup=10 ** 9)  # (the twin never captures)
                it, losses = iter(host), []
                for step in range(n_steps):
                    if graphs and step == 3:
                        pipe._warmup = 0  # three eager steps lie behind: steps 3 and 4 capture their slot and replay, 5 and 6 replay
                    l, _, _ = pipe.progress(it)
                    assert list(l) == ["binary_cross_entropy"]
                    losses.append(l["binary_cross_entropy"].detach().clone())
                torch.cuda.synchronize()
                assert (pipe._graphs[0] is not None and pipe._graphs[1] is not None) == graphs  # captured without raising
                res.append((torch.stack(losses).cpu(), {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()},
                            {n: p.detach().cpu().clone() for n, p in model.named_parameters() if not n.startswith("embedding_group.")}))
    finally:
        for nm in ENTRY_POINTS:
            setattr(lib, nm, orig[nm])
    # two layers x 2 entry points each way per recorded step (7 eager steps, then 3 eager + 2 captured; replays call nothing)
    assert calls == [2 * 2 * (7 + 5), 2 * 2 * (7 + 5)], calls
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la.tolist(), "eager then replayed", lb.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    assert len(pa) == 31
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
