"""torch.ops.tzrec_hip.hstu_mha_fwd / _bwd (torcheasyrec_amd/ops.py) against the float64 form of tests/hstu_ref.py under the
project's bound, through the registered autograd formula and `opcheck` -- a batch of ONE row among the cases (its gradient slices
are contiguous as they lie; its upstream gradient may carry any row stride) -- and the autograd function captured into a graph."""
import pytest
import torch

import hstu_ref as ref
from torcheasyrec_amd import _lib

BLK, TILE = _lib.HSTU_BLOCK, _lib.HSTU_TILE
CASES = {"one_row": ([1], None, 0), "edges": ([0, TILE + 1, BLK + 1], [0, 3, TILE + 1], 2)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_ops_against_float64_and_opcheck(dev, name):
    from torcheasyrec_amd import ops  # noqa: F401  (registers the ops)

    lengths, targets, c = CASES[name]
    p, want = ref.draw(lengths, 2, 8, 12, 2 * BLK + 8, 200 + sorted(CASES).index(name), targets, 0, c)
    q, k, v = (p[x].to(dev).requires_grad_(True) for x in "qkv")
    nt = None if targets is None else p["num_targets"].to(dev)
    args = (p["offsets"].to(dev), nt, p["max_seq_len"], p["alpha"], 0, c, -1)
    wide = torch.zeros(q.shape[0], 2 * 12 + 1, device=dev)  # the upstream gradient with an odd number of floats between its rows
    wide[:, :24] = p["g"].to(dev).reshape(-1, 24)
    g = wide[:, :24].view(-1, 2, 12)
    out = torch.ops.tzrec_hip.hstu_mha_fwd(q, k, v, *args)
    dq, dk, dv = torch.autograd.grad(out, [q, k, v], g)  # through the registered formula = hstu_mha_bwd
    ref.check({"out": [out.detach()], "dq": [dq], "dk": [dk], "dv": [dv]}, want, ref.gaps(p, want), f"ops {name} on {dev.type}", ref.KINDS)
    if dev.type == "cpu":  # opcheck: schema, fake impl vs real, no aliasing among the returns, autograd registration, aot dispatch
        torch.library.opcheck(torch.ops.tzrec_hip.hstu_mha_fwd, (q, k, v, *args))
        torch.library.opcheck(torch.ops.tzrec_hip.hstu_mha_bwd, (g, q.detach(), k.detach(), v.detach(), *args))


def test_captured_graph_replays_equal_the_eager_runs(dev):
    from torcheasyrec_amd import hstu

    if dev.type != "cuda":
        return  # (the emulator has no graphs)
    lengths, targets = [0, 1, TILE + 1, BLK + 1, 2 * BLK + 1], [0, 0, 3, TILE + 1, 5]
    draws = [ref.draw(lengths, 2, 8, 12, 2 * BLK + 8, seed, targets, TILE + 4, 3)[0] for seed in (210, 211)]
    p = draws[0]
    offsets, nt = p["offsets"].to(dev), p["num_targets"].to(dev)
    held_in = [torch.zeros_like(p[x], device=dev).requires_grad_(x != "g") for x in "qkvg"]

    def load(i):
        with torch.no_grad():
            for dst, x in zip(held_in, "qkvg"):
                dst.copy_(draws[i][x])

    def step():
        q, k, v, g = held_in
        out = hstu.hstu_mha(p["max_seq_len"], p["alpha"], q, k, v, offsets, num_targets=nt, max_attn_len=p["L"], contextual_seq_len=p["c"])
        return (out.detach(),) + torch.autograd.grad(out, [q, k, v], g)

    eager = []
    for i in (0, 1):
        load(i)
        eager.append([t.clone() for t in step()])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for i in (0, 1, 1, 0):  # several replays, on fresh inputs and on the same ones again
        load(i)
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(held, eager[i]))
