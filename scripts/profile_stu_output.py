"""The STU layer's output stage (csrc/stu_output.hip, hstu.FUSED_STU_OUTPUT) against the literal form (hstu.stu_output_literal:
silu, layer norm, the product, the concat, dropout, addmm, and their autograd), on the same box in the same process, one forward +
backward on the same inputs:

    L = 38 866 rows (the rows of scripts/profile_hstu_attention.py), H = 4, Dv = 128, E = 512, layer norm, p = 0.3 training, u
    the first H Dv columns of a [L, (2 Dv + 2 Da) H] uvqk matrix.

    python scripts/profile_stu_output.py time [out.json]       one device-event pair per pass, RUNS passes per form after WARM
                                                               warm-up passes of each, the forms ALTERNATING with nothing in
                                                               between -- fused and literal, each eager and replayed from a
                                                               hipGraph -- min / median / max per form, the peak memory of one
                                                               pass, and replays with a GIVEN seed against the eager result
    python scripts/profile_stu_output.py trace fused|literal   ITERS eager passes and nothing else: run under `rocprofv3
                                                               --kernel-trace --stats`, one run per form"""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, hstu  # noqa: E402

L, H, DV, DA, E, P = 38866, 4, 128, 128, 512, 0.3
WARM, RUNS, ITERS = 3, 40, 5


def make_pass(dev, seed=None):
    torch.manual_seed(0)
    W = H * DV
    uvqk = torch.randn(L, (2 * DV + 2 * DA) * H, device=dev).requires_grad_(True)
    attn, x = torch.randn(L, W, device=dev).requires_grad_(True), torch.randn(L, E, device=dev).requires_grad_(True)
    gamma, beta = (1 + 0.1 * torch.randn(W, device=dev)).requires_grad_(True), (0.1 * torch.randn(W, device=dev)).requires_grad_(True)
    wo = (torch.randn(3 * W, E, device=dev) / (3 * W) ** 0.5).requires_grad_(True)
    g = torch.randn(L, E, device=dev)

    def run():
        out = hstu.stu_output(uvqk[:, :W], attn, x, gamma, beta, wo, H, False, P, True, seed=seed)
        return torch.autograd.grad(out, [uvqk, attn, x, gamma, beta, wo], g)

    return run


def form(run, fused):
    def f():
        hstu.FUSED_STU_OUTPUT = fused
        return run()
    return f


def captured(f):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = f()
    return graph, keep


def peak_bytes(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del g
    return peak


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = hstu.FUSED_STU_OUTPUT
    _lib.use_native()
    dev = torch.device("cuda", 0)
    run = make_pass(dev)
    if mode == "trace":
        f = form(run, sys.argv[2] == "fused")
        for _ in range(ITERS):
            f()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes")
        return
    peaks = {"fused": peak_bytes(form(run, True)), "literal": peak_bytes(form(run, False))}
    graphs = {"fused": captured(form(run, True)), "literal": captured(form(run, False))}
    forms = {"fused_replayed": graphs["fused"][0].replay, "fused_eager": form(run, True), "literal_replayed": graphs["literal"][0].replay,
             "literal_eager": form(run, False)}
    for _ in range(WARM):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in forms}
    for _ in range(RUNS):  # alternating pass by pass: every form sees the same box in the same state
        for k, f in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    # a given seed: every replay must give the eager result, bit for bit
    fixed = form(make_pass(dev, torch.tensor([12345], device=dev)), True)
    eager = [t.clone() for t in fixed()]
    graph, keep = captured(fixed)
    same = True
    for _ in range(3):
        graph.replay()
        same = same and all(bool(torch.equal(a, b)) for a, b in zip(keep, eager))
    us = {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}
    out = {"rows": L, "H": H, "Dv": DV, "E": E, "p": P, "norm": "layer",
           "mode": "forward + backward, u a column slice of one uvqk matrix; each form eager and replayed from a hipGraph",
           "warm_up_passes": WARM, "timed_passes": RUNS, "us_per_pass": {k: {"min": v[0], "median": v[len(v) // 2], "max": v[-1]} for k, v in us.items()},
           "peak_bytes": peaks, "replays_with_a_given_seed_equal_eager": same}
    hstu.FUSED_STU_OUTPUT = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
