"""HSTU's jagged attention (csrc/hstu_attention.hip, hstu.FUSED_HSTU_MHA) against the literal padded form (hstu.hstu_mha_literal: pad
to [B, H, N, .], the [B, H, N, N] scores, mask, SiLU, the product with v, back to the rows, and their autograd), on the same box in
the same process, one forward + backward on the same inputs:

    B = 16 sequences of 0 .. 4096 rows (uniform), max_seq_len 4096, H = 4, Da = Dv = 128, 0 .. 8 targets a sample, a contextual
    prefix of 4 rows, alpha = 128^-1/2.  B and max_seq_len are set by the LITERAL form: each of its [B, H, N, N] fp32 tensors is
    4.3 GB at this pair, and its forward + backward holds several at once.

    python scripts/profile_hstu_attention.py time [out.json]       one device-event pair per pass, RUNS passes per form after WARM
                                                                   warm-up passes of each, the forms ALTERNATING with nothing in
                                                                   between -- fused replayed from a hipGraph, fused eager, literal
                                                                   eager (it does not capture: its scatter back to the rows reads
                                                                   a mask back) -- the median per form, the peak memory of one
                                                                   pass, and the replayed gradient against the eager one
    python scripts/profile_hstu_attention.py trace fused|literal   ITERS eager passes and nothing else: run under `rocprofv3
                                                                   --kernel-trace --stats`, one run per form"""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, hstu  # noqa: E402

B, N, H, DA, DV, CONTEXTUAL, MAX_TARGETS = 16, 4096, 4, 128, 128, 4, 8
WARM, RUNS, ITERS = 3, 40, 5


def make_pass(dev):
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(0, N + 1, (B,), generator=gen)
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)]).to(dev)
    targets = torch.minimum(torch.randint(0, MAX_TARGETS + 1, (B,), generator=gen), lens).to(dev)
    L = int(lens.sum())
    torch.manual_seed(0)
    # q, k, v where the uvqk product leaves them: column slices of one [L, (2 Dv + 2 Da) H] matrix
    uvqk = torch.randn(L, (2 * DV + 2 * DA) * H, device=dev).requires_grad_(True)
    g = torch.randn(L, H, DV, device=dev)

    def run():
        _, v, q, k = torch.split(uvqk, [DV * H, DV * H, DA * H, DA * H], dim=1)
        out = hstu.hstu_mha(N, DA ** -0.5, q.view(L, H, DA), k.view(L, H, DA), v.view(L, H, DV), offsets, num_targets=targets,
                            contextual_seq_len=CONTEXTUAL)
        return torch.autograd.grad(out, [uvqk], g)

    return run, int((lens.double() ** 2).sum()), L


def captured(run):
    hstu.FUSED_HSTU_MHA = True
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = run()
    return graph, keep


def peak_bytes(run, fused):
    hstu.FUSED_HSTU_MHA = fused
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del g
    return peak


def form_grad(run):
    hstu.FUSED_HSTU_MHA = True
    return run()[0]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = hstu.FUSED_HSTU_MHA
    _lib.use_native()
    run, pairs, L = make_pass(torch.device("cuda", 0))
    if mode == "trace":
        hstu.FUSED_HSTU_MHA = sys.argv[2] == "fused"
        for _ in range(ITERS):
            run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes")
        return
    peaks = {"fused": peak_bytes(run, True), "literal": peak_bytes(run, False)}

    def form(fused):
        def f():
            hstu.FUSED_HSTU_MHA = fused
            run()
        return f

    graph, keep = captured(run)
    forms = {"fused_replayed": graph.replay, "fused_eager": form(True), "literal_eager": form(False)}
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
    graph.replay()
    replay_equals_eager = bool(torch.equal(keep[0], form_grad(run)))
    us = {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}
    out = {"B": B, "max_seq_len": N, "H": H, "Da": DA, "Dv": DV, "contextual_seq_len": CONTEXTUAL, "max_targets": MAX_TARGETS, "rows": L,
           "sum_n_squared": pairs, "padded_pairs": B * N * N, "mode": "forward + backward, q / k / v column slices of one uvqk matrix; fused replayed from a hipGraph and eager, literal eager (it does not capture)",
           "warm_up_passes": WARM, "timed_passes": RUNS, "us_per_pass": {k: {"min": v[0], "median": v[len(v) // 2], "max": v[-1]} for k, v in us.items()},
           "peak_bytes": peaks, "replay_equals_eager": replay_equals_eager}
    hstu.FUSED_HSTU_MHA = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
