"""DAT's Adaptive-Mimic loss (csrc/amm_loss.hip, match.amm_loss) against the reference's literal op sequence
(match.FUSED_AMM_LOSS = False: per side normalize -- norm, clamp, expand, divide --, slice, subtract, square, sum, multiply, with
sample weights a multiply, two means and the div_no_nan; then autograd's backward of all of it) on the same box in the same process,
both sides, forward + backward on the same inputs:

    B = 8192, D = 64, COSINE, 12 sampled negatives behind the positives on the item side, amm_u_weight = amm_i_weight = 0.5; once
    without sample weights and once with; the two augment tensors get their gradient

    python scripts/profile_amm_loss.py time [out.json]      each form's pass is captured into a hipGraph of its own; one device-event
                                                            pair per replay, RUNS replays per form after WARM warm-up replays of
                                                            each, fused and literal ALTERNATING replay by replay with nothing in
                                                            between (the device stays busy); the median per form
    python scripts/profile_amm_loss.py trace fused|literal  ITERS eager forward + backward passes of both settings and nothing else:
                                                            run under `rocprofv3 --kernel-trace --stats`, one run per form (no counters
                                                            in the same run); launches / ITERS is the launch count of a pass"""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, match  # noqa: E402

B, D, NEG, C_U, C_I = 8192, 64, 12, 0.5, 0.5
WARM, RUNS, ITERS = 10, 60, 20


def amm_pass(dev, weights):
    torch.manual_seed(1 if weights else 0)
    ua = torch.randn(B, D, device=dev).requires_grad_(True)
    ia = torch.randn(B + NEG, D, device=dev).requires_grad_(True)
    ue, ie = torch.randn(B, D, device=dev), torch.randn(B + NEG, D, device=dev)
    w = (0.5 + torch.rand(B, device=dev)) if weights else None
    g = [torch.tensor(1.0, device=dev), torch.tensor(1.0, device=dev)]
    assert match.amm_loss_ok(ua, ia, ue, ie, w)

    def run():
        return torch.autograd.grad(list(match.amm_loss(ua, ia, ue, ie, True, C_U, C_I, w)), [ua, ia], g)

    return run


def captured(run, fused):
    """the pass of one form as a hipGraph: three eager passes on a side stream, then the capture"""
    match.FUSED_AMM_LOSS = fused
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
    default = match.FUSED_AMM_LOSS
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {"no_weights": amm_pass(dev, False), "weights": amm_pass(dev, True)}
    if mode == "trace":
        match.FUSED_AMM_LOSS = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    out = {"B": B, "D": D, "sampled_negatives": NEG, "cosine": True, "amm_u_weight": C_U, "amm_i_weight": C_I, "warm_up_replays": WARM,
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
    match.FUSED_AMM_LOSS = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
