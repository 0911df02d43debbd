"""tests/golden/xdeepfm_mini.config through GraphTrainPipeline at B = 64: three eager steps followed by four steps captured into /
replayed from hipGraphs leave bit for bit what seven eager steps of an identically seeded twin leave -- the forward launch of
the CIN, the backward's 2 L + 1 launches, the saved activations they overwrite and the workspace all capture (the host arrays
of pointers and sizes are read when the launch is recorded), nothing reads the device.  And the memory condition the fused
CIN exists for: no tensor of the size of z = einsum("bhd,bfd->bhfd") is allocated, forward or backward."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.gpu
def test_xdeepfm_replays_from_a_graph():
    from examples.train_from_config import synthetic_batches
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import GraphTrainPipeline
    from torcheasyrec_amd.rank_model import ConfigXDeepFM, build_rank_model

    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(open(os.path.join(os.path.dirname(__file__), "golden", "xdeepfm_mini.config")).read())
    B, n_steps = 64, 7
    host = [b.pin_memory() for b in synthetic_batches(spec, n_steps * B, B, seed=9)]
    res = []
    work = torch.cuda.Stream(dev)
    with torch.cuda.stream(work):
        for graphs in (False, True):
            torch.manual_seed(3)
            model = build_rank_model(spec, device=dev)
            assert type(model) is ConfigXDeepFM
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
    (la, ta, pa), (lb, tb, pb) = res
    print("losses eager", la.tolist(), "eager then replayed", lb.tolist())
    assert bool(torch.isfinite(la).all()) and torch.equal(la, lb)
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    assert len(pa) == 12
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n


@pytest.mark.gpu
def test_cin_allocates_no_tensor_of_the_size_of_z():
    """B = 2048, F = 26, D = 16, [64, 64]: the growth of torch.cuda.max_memory_allocated() over a CIN forward + backward stays
    below a quarter of the first layer's z (B F F D 4 = 88.6 MB -> 22.1 MB).  Counted: y, the saved X^1 (8.4 MB, which the
    backward overwrites with dX^1), gx, the weight and bias gradients and the backward's workspace, which comes from
    _lib.workspace, i.e. from torch's allocator (12 and 4 parts of the two layers' weight gradients, 3.8 MB).  The literal form allocates both
    z (88.6 + 218 MB) and has to exceed the limit, or the measurement measures nothing."""
    from torcheasyrec_amd import _lib, interaction
    from torcheasyrec_amd.interaction import CIN

    _lib.use_native()
    dev = torch.device("cuda", 0)
    B, F, D, layers = 2048, 26, 16, [64, 64]
    limit = B * F * F * D * 4 // 4
    torch.manual_seed(0)
    m = CIN(F, layers).to(dev)
    x = (0.5 * torch.randn(B, F, D, device=dev)).requires_grad_(True)
    gy = torch.randn(B, sum(layers), device=dev)
    growth = {}
    try:
        for fused in (True, False):
            interaction.FUSED_CIN = fused
            for _ in range(2):  # (the second pass: the parameters' .grad exist already, as in training)
                x.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                m(x).backward(gy)
                torch.cuda.synchronize()
                growth[fused] = torch.cuda.max_memory_allocated(dev) - before
    finally:
        interaction.FUSED_CIN = True
    print(f"peak growth: fused {growth[True] / 1e6:.1f} MB, literal {growth[False] / 1e6:.1f} MB, limit {limit / 1e6:.1f} MB")
    assert growth[True] < limit
    assert growth[False] > limit
