"""The gate-and-mix step of a CGC level of PLE (tzr_cgc_mix_*, csrc/gate_mix.hip) against the reference's literal stack / softmax / matmul form
(ple.FUSED_CGC_MIX = False) on the same box in the same run, forward + backward at B = 8192, at the first two levels of the
reference's docs example (docs/source/models/ple.md), both with a shared gate:

    H = 256, T = 2, P = 2, S = 2   (6 experts, 3 gates; experts [1024, 512, 256] over a 512-wide input)
    H = 64,  T = 2, P = 3, S = 3   (9 experts, 3 gates; experts [256, 128, 64] over a 256-wide input)

each as the mixing step alone (logits and expert outputs given) and as the whole `ExtractionNet` (experts and gates included).

    python scripts/profile_cgc_mix.py time [out.json]      device events, fused and literal alternating, spread over rounds
    python scripts/profile_cgc_mix.py trace fused|literal  ITERS forward + backward passes of the mixing step of every shape and
                                                            nothing else: run under `rocprofv3 --kernel-trace --stats`, one pass
                                                            per form (no counters in the same run); launches / ITERS and the sum
                                                            of the kernel times / ITERS are the launch count and device time of a pass

Bytes a fused pass has to move, from the shapes (E experts, G gates, n = sum of the gates' member counts): forward
(E + G) B H 4 + 2 n B 4; backward (2 E + G) B H 4 + 2 n B 4."""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, ple  # noqa: E402
from torcheasyrec_amd.ple import ExtractionNet  # noqa: E402

B = 8192
# (H, T, P, S, input width, expert hidden units)
SHAPES = [(256, 2, 2, 2, 512, [1024, 512, 256]), (64, 2, 3, 3, 256, [256, 128, 64])]
ITERS = 50


def bytes_moved(H, T, P, S):
    E, G, n = T * P + S, T + 1, T * (P + S) + T * P + S
    return {"fwd": (E + G) * B * H * 4 + 2 * n * B * 4, "bwd": (2 * E + G) * B * H * 4 + 2 * n * B * 4}


def mix_pass(dev, H, T, P, S):
    """the level's own code path with the experts and gate logits given: ExtractionNet.forward's mixing step"""
    from torcheasyrec_amd.gate_ops import cgc_mix, cgc_mix_ok

    torch.manual_seed(0)
    shared = list(range(T * P, T * P + S))
    sels = [list(range(t * P, (t + 1) * P)) + shared for t in range(T)] + [list(range(T * P)) + shared]
    experts = [torch.randn(B, H, device=dev).requires_grad_(True) for _ in range(T * P + S)]
    logits = [torch.randn(B, len(s), device=dev).requires_grad_(True) for s in sels]
    gouts = [torch.randn(B, H, device=dev) for _ in sels]
    assert cgc_mix_ok(logits, experts, sels)

    def run():
        if ple.FUSED_CGC_MIX:
            outs = cgc_mix(logits, experts, sels)
        else:
            outs = [torch.matmul(torch.softmax(lg, dim=1).unsqueeze(1), torch.stack([experts[e] for e in sel], dim=1)).squeeze(1)
                    for lg, sel in zip(logits, sels)]
        torch.autograd.grad(outs, logits + experts, gouts)

    return run


def level_pass(dev, H, T, P, S, d_in, hidden):
    torch.manual_seed(0)
    net = ExtractionNet([d_in] * T, d_in, "level", S, P, {"hidden_units": hidden}, {"hidden_units": hidden}).to(dev)
    xs = [(0.5 * torch.randn(B, d_in, device=dev)).requires_grad_(True) for _ in range(T + 1)]
    gouts = [torch.randn(B, H, device=dev) for _ in range(T + 1)]

    def run():
        for p in net.parameters():
            p.grad = None
        for x in xs:
            x.grad = None
        outs, shared = net(xs[:T], xs[T])
        torch.autograd.backward(list(outs) + [shared], gouts)

    return run


def timed(run, fused, n):
    ple.FUSED_CGC_MIX = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = ple.FUSED_CGC_MIX
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {f"mix H={H} T={T} P={P} S={S}": mix_pass(dev, H, T, P, S) for H, T, P, S, _, _ in SHAPES}
    if mode == "trace":
        ple.FUSED_CGC_MIX = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    for H, T, P, S, d_in, hidden in SHAPES:
        work[f"ExtractionNet H={H} T={T} P={P} S={S}"] = level_pass(dev, H, T, P, S, d_in, hidden)
    out = {"B": B, "iters_per_round": ITERS, "bytes": {f"H={H} T={T} P={P} S={S}": bytes_moved(H, T, P, S) for H, T, P, S, _, _ in SHAPES},
           "us_per_pass": {}}
    for name, run in work.items():
        for fused in (True, False):  # warm-up of both forms
            timed(run, fused, 10)
        rounds = {"fused": [], "literal": []}
        for _ in range(6):  # alternating: both forms see the same box
            rounds["fused"].append(timed(run, True, ITERS))
            rounds["literal"].append(timed(run, False, ITERS))
        out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
        print(name, json.dumps(out["us_per_pass"][name]), flush=True)
    ple.FUSED_CGC_MIX = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
