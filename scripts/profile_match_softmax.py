"""The match models' similarity head (csrc/match_softmax.hip) against the reference's literal form -- two F.normalize, the
positive's multiply-and-sum, the negatives' matmul, cat, divide, CrossEntropyLoss (match.FUSED_MATCH_SOFTMAX = False) -- on the
same box in the same process, forward + backward on the same tower outputs, at the example's shape (examples/dssm_taobao.config:
batch_size 8192, output_dim 64, COSINE, temperature 0.05) in both modes:

    sampled    B = 8192, N = 1024 negatives: a [8192, 1025] score matrix, 32 MiB a copy
    in_batch   B = 8192: [8192, 8192], 256 MiB a copy

The towers' outputs are given (leaves); both get their gradient.  Neither form returns the score matrix (want_sim off).

    python scripts/profile_match_softmax.py time [out.json]      one device-event pair per pass, RUNS passes per form after WARM
                                                                  warm-up passes of each, fused and literal ALTERNATING pass by
                                                                  pass with nothing in between (the device stays busy); the
                                                                  median per form, and torch.cuda.max_memory_allocated of one
                                                                  forward + backward per form above what the inputs take
    python scripts/profile_match_softmax.py trace fused|literal  ITERS forward + backward passes of both shapes and nothing else:
                                                                  run under `rocprofv3 --kernel-trace --stats`, one pass per
                                                                  form (no counters in the same run); launches / ITERS and the
                                                                  sum of the kernel times / ITERS are the launch count and
                                                                  device time of a pass"""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, match  # noqa: E402

B, N, D, T = 8192, 1024, 64, 0.05
WARM, RUNS, ITERS = 10, 60, 20
SHAPES = {"sampled": (match.SAMPLED, B + N), "in_batch": (match.IN_BATCH, B)}


def head_pass(dev, mode, M):
    torch.manual_seed(0)
    u = torch.randn(B, D, device=dev).requires_grad_(True)
    v = torch.randn(M, D, device=dev).requires_grad_(True)
    assert match.match_softmax_ok(u, v, mode)

    def run():
        loss, _, _ = match.match_softmax(u, v, mode, True, T)
        return torch.autograd.grad(loss, [u, v])

    return run


def one(run, fused):
    match.FUSED_MATCH_SOFTMAX = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    return a, b


def peak_bytes(run, fused):
    match.FUSED_MATCH_SOFTMAX = fused
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del g
    return peak


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = match.FUSED_MATCH_SOFTMAX
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {name: head_pass(dev, *shape) for name, shape in SHAPES.items()}
    if mode == "trace":
        match.FUSED_MATCH_SOFTMAX = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    out = {"B": B, "N": N, "D": D, "temperature": T, "similarity": "COSINE", "warm_up_passes": WARM, "timed_passes": RUNS,
           "score_matrix_bytes": {"sampled": B * (1 + N) * 4, "in_batch": B * B * 4}, "us_per_pass": {}, "peak_bytes": {}}
    for name, run in work.items():
        for fused in (True, False):
            for _ in range(WARM):
                one(run, fused)
        torch.cuda.synchronize()
        ev = {"fused": [], "literal": []}
        for _ in range(RUNS):  # alternating pass by pass: both forms see the same box in the same state
            ev["fused"].append(one(run, True))
            ev["literal"].append(one(run, False))
        torch.cuda.synchronize()
        us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in ev.items()}
        out["us_per_pass"][name] = {k: {"min": min(v), "median": median(v), "max": max(v)} for k, v in us.items()}
        out["peak_bytes"][name] = {"fused": peak_bytes(run, True), "literal": peak_bytes(run, False)}
        print(name, json.dumps(out["us_per_pass"][name]), json.dumps(out["peak_bytes"][name]), flush=True)
    match.FUSED_MATCH_SOFTMAX = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
