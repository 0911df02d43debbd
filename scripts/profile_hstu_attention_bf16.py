"""HSTU's jagged attention in bf16 (csrc/hstu_attention_bf16.hip, hstu.FUSED_HSTU_MHA_BF16) against the literal padded form in bf16
and against the fp32 kernels (csrc/hstu_attention.hip), on the same box in the same process, one forward + backward a pass at the
shape of scripts/profile_hstu_attention.py:

    B = 16 sequences of 0 .. 4096 rows (uniform), max_seq_len 4096, H = 4, Da = Dv = 128, 0 .. 8 targets a sample, a contextual
    prefix of 4 rows, alpha = 128^-1/2, q / k / v column slices of one uvqk matrix (bf16 for the two bf16 forms, fp32 for the third).

    python scripts/profile_hstu_attention_bf16.py time [out.json]     one device-event pair per pass, RUNS passes per form after WARM
                                                                      warm-up passes of each, the three forms ALTERNATING pass by
                                                                      pass, all eager: the median and range per form, the peak
                                                                      memory of one pass, the bf16 rate end to end from the shapes
    python scripts/profile_hstu_attention_bf16.py trace fused|literal ITERS eager bf16 passes and nothing else: run under `rocprofv3
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


def make_pass(dev, dtype, bf16_fused):
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(0, N + 1, (B,), generator=gen)
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)]).to(dev)
    targets = torch.minimum(torch.randint(0, MAX_TARGETS + 1, (B,), generator=gen), lens).to(dev)
    L = int(lens.sum())
    torch.manual_seed(0)
    uvqk = torch.randn(L, (2 * DV + 2 * DA) * H, device=dev).to(dtype).requires_grad_(True)
    g = torch.randn(L, H, DV, device=dev).to(dtype)

    def run():
        hstu.FUSED_HSTU_MHA_BF16 = bf16_fused
        before = hstu._HstuMhaFn.calls
        _, v, q, k = torch.split(uvqk, [DV * H, DV * H, DA * H, DA * H], dim=1)
        out = hstu.hstu_mha(N, DA ** -0.5, q.view(L, H, DA), k.view(L, H, DA), v.view(L, H, DV), offsets, num_targets=targets,
                            contextual_seq_len=CONTEXTUAL)
        assert hstu._HstuMhaFn.calls == before + (1 if bf16_fused or dtype == torch.float32 else 0)
        return torch.autograd.grad(out, [uvqk], g)

    return run, int((lens.double() ** 2).sum()), L


def peak_bytes(run):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del g
    return peak


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = hstu.FUSED_HSTU_MHA_BF16
    _lib.use_native()
    dev = torch.device("cuda", 0)
    if mode == "trace":
        run, _, _ = make_pass(dev, torch.bfloat16, sys.argv[2] == "fused")
        for _ in range(ITERS):
            run()
        torch.cuda.synchronize()
        print(f"bf16 {sys.argv[2]}: {ITERS} forward + backward passes")
        return
    forms = {"bf16_fused": make_pass(dev, torch.bfloat16, True), "bf16_literal": make_pass(dev, torch.bfloat16, False),
             "fp32_fused": make_pass(dev, torch.float32, True)}
    pairs, L = forms["bf16_fused"][1:]
    forms = {k: f[0] for k, f in forms.items()}
    peaks = {k: peak_bytes(f) for k, f in forms.items()}
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
    us = {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}
    # the products of a pass over the causal half of sum n^2 pairs a head: forward 2 (Da + Dv), row pass 2 (2 Da + Dv), column pass
    # 2 (2 Da + 2 Dv) flops a pair (scores and dP recomputed in both backward passes)
    flops = 0.5 * pairs * H * 2 * ((DA + DV) + (2 * DA + DV) + (2 * DA + 2 * DV))
    out = {"B": B, "max_seq_len": N, "H": H, "Da": DA, "Dv": DV, "contextual_seq_len": CONTEXTUAL, "max_targets": MAX_TARGETS, "rows": L,
           "sum_n_squared": pairs, "mode": "forward + backward, eager, q / k / v column slices of one uvqk matrix; three forms alternating pass by pass",
           "warm_up_passes": WARM, "timed_passes": RUNS, "us_per_pass": {k: {"min": v[0], "median": v[len(v) // 2], "max": v[-1]} for k, v in us.items()},
           "peak_bytes": peaks, "causal_flops_per_pass": flops,
           "bf16_fused_tflops_end_to_end": flops / (us["bf16_fused"][len(us["bf16_fused"]) // 2] * 1e-6) / 1e12}
    hstu.FUSED_HSTU_MHA_BF16 = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
