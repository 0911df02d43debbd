"""Rocket Launching's distillation terms (csrc/distill_loss.hip, rocket.distill_losses) against the reference's literal op sequence
(rocket.FUSED_DISTILL_LOSS = False: per layer pair two normalize -- norm, clamp, expand, divide --, multiply, row sum, with sample
weights a multiply, mean, scale; the hint's MSELoss, with weights a multiply and a mean, and the div_no_nan; then autograd's backward
of all of it) on the same box in the same process, forward + backward on the same inputs:

    the Criteo example's shape (examples/rocket_launching_criteo.config): B = 8192, two layer pairs of widths 64 and 32, COSINE;
    once without sample weights on [B, 2] logits (num_class 2) and once with weights on [B] logits (num_class 1: the model refuses
    weights with more classes); the light tensors and the light logits get their gradient

    python scripts/profile_distill_loss.py time [out.json]   each form's pass is captured into a hipGraph of its own; one
                                                             device-event pair per replay, RUNS replays per form after WARM warm-up
                                                             replays of each, fused and literal ALTERNATING replay by replay with
                                                             nothing in between (the device stays busy); the median per form
    python scripts/profile_distill_loss.py trace fused|literal no_weights|weights
                                                             ITERS eager forward + backward passes of that form and setting and nothing
                                                             else: run under `rocprofv3 --kernel-trace --stats`, one run each (no
                                                             counters in the same run); launches / ITERS is the launch count of a pass"""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, rocket  # noqa: E402

B, WIDTHS = 8192, (64, 32)
WARM, RUNS, ITERS = 10, 60, 20


def distill_pass(dev, weights):
    torch.manual_seed(1 if weights else 0)
    ls = [torch.randn(B, W, device=dev).requires_grad_(True) for W in WIDTHS]
    bs = [torch.randn(B, W, device=dev) for W in WIDTHS]
    shape = (B,) if weights else (B, 2)
    ll, lb = torch.randn(*shape, device=dev).requires_grad_(True), torch.randn(*shape, device=dev)
    w = (0.5 + torch.rand(B, device=dev)) if weights else None
    g = [torch.tensor(1.0, device=dev) for _ in range(len(WIDTHS) + 1)]
    assert rocket.distill_losses_ok(ls, bs, ll, lb, w)

    def run():
        sims, hint = rocket.distill_losses(ls, bs, ll, lb, True, w)
        return torch.autograd.grad(list(sims) + [hint], ls + [ll], g)

    return run


def captured(run, fused):
    """the pass of one form as a hipGraph: three eager passes on a side stream, then the capture"""
    rocket.FUSED_DISTILL_LOSS = fused
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = run()
    return graph, keep


def one(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    return a, b


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = rocket.FUSED_DISTILL_LOSS
    _lib.use_native()
    dev = torch.device("cuda", 0)
    if mode == "trace":
        rocket.FUSED_DISTILL_LOSS = sys.argv[2] == "fused"
        run = distill_pass(dev, sys.argv[3] == "weights")
        for _ in range(ITERS):
            run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]} {sys.argv[3]}: {ITERS} forward + backward passes")
        return
    work = {"no_weights": distill_pass(dev, False), "weights": distill_pass(dev, True)}
    out = {"B": B, "pair_widths": list(WIDTHS), "cosine": True, "logits": {"no_weights": [B, 2], "weights": [B]}, "warm_up_replays": WARM,
           "timed_replays": RUNS, "timing": "hipGraph replay, device events", "us_per_pass": {}}
    for name, run in work.items():
        graphs = {"fused": captured(run, True), "literal": captured(run, False)}
        for _ in range(WARM):
            for g, _keep in graphs.values():
                one(g)
        torch.cuda.synchronize()
        same = max(float((a - b).abs().max()) for a, b in zip(graphs["fused"][1], graphs["literal"][1]))  # (what the replays left)
        ev = {"fused": [], "literal": []}
        for _ in range(RUNS):  # alternating replay by replay: both forms see the same box in the same state
            for k in ev:
                ev[k].append(one(graphs[k][0]))
        torch.cuda.synchronize()
        us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in ev.items()}
        out["us_per_pass"][name] = {k: {"min": min(v), "median": median(v), "max": max(v)} for k, v in us.items()}
        out["us_per_pass"][name]["max_abs_gradient_difference"] = same
        print(name, json.dumps(out["us_per_pass"][name]), flush=True)
    rocket.FUSED_DISTILL_LOSS = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
