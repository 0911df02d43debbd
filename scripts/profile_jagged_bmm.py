"""The jagged matmul with per-sample weights (csrc/jagged_bmm.hip, hstu_mlps.FUSED_JAGGED_BMM) on the skewed batch of
scripts/profile_hstu_position.py (its lengths and seed): B = 16 samples of 0 .. 4096 rows, 38 866 rows in all, N = 512 STU columns,
at K = 64 (the action MLP of the kuairand configs: 8 actions x 8) and K = 256.  One forward plus backward (out, then d jagged,
d dense and d bias under a fixed g), fp32, two forms a shape:

    K64_fused / K64_literal / K256_fused / K256_literal      the kernels against hstu_mlps' own literal (padded) form

    python scripts/profile_jagged_bmm.py time [out.json]   RUNS device-event pairs a form after WARM warm-up passes, the forms
                                                            ALTERNATING pass by pass; median, minimum and maximum, the peak
                                                            memory of one pass, and per shape whether the fused range lies
                                                            wholly below the literal one
    python scripts/profile_jagged_bmm.py trace FORM        ITERS passes and nothing else: run under `rocprofv3 --kernel-trace --stats`"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from torcheasyrec_amd import _build, _lib, hstu_mlps  # noqa: E402

B, MAX_SEQ_LEN, N, KS = 16, 4096, 512, (64, 256)
WARM, RUNS, ITERS = 3, 40, 5
KINDS = ("out", "d_jagged", "d_dense", "d_bias")


def make_passes(dev):
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(0, MAX_SEQ_LEN + 1, (B,), generator=gen)
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)]).to(dev)
    L = int(lens.sum())
    torch.manual_seed(0)
    g = torch.randn(L, N, device=dev)
    passes = {}
    for K in KS:
        x, w, b = (t.requires_grad_(True) for t in (torch.randn(L, K, device=dev), torch.randn(B, K, N, device=dev) * K ** -0.5, torch.randn(B, N, device=dev)))
        for fname, fused in (("fused", True), ("literal", False)):
            def run(x=x, w=w, b=b, fused=fused):
                hstu_mlps.FUSED_JAGGED_BMM = fused
                out = hstu_mlps.jagged_dense_bmm_broadcast_add(MAX_SEQ_LEN, offsets, x, w, b)
                return (out, *torch.autograd.grad(out, [x, w, b], g))
            passes[f"K{K}_{fname}"] = run
    return passes, lens.tolist(), L


def peak_bytes(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    _lib.use_library(_build.build())
    assert _lib.backend().startswith("hip")
    passes, lens, L = make_passes(torch.device("cuda", 0))
    if mode == "trace":
        for _ in range(ITERS):
            passes[sys.argv[2]]()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} passes")
        return
    before = hstu_mlps._JaggedBmmFn.calls
    outs = {k: f() for k, f in passes.items()}
    assert hstu_mlps._JaggedBmmFn.calls == before + len(KS)
    diff = {f"K{K}": {k: float((a - b).abs().max()) for k, a, b in zip(KINDS, outs[f"K{K}_fused"], outs[f"K{K}_literal"])} for K in KS}
    del outs
    peaks = {k: peak_bytes(f) for k, f in passes.items()}
    for _ in range(WARM):
        for f in passes.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in passes}
    for _ in range(RUNS):  # alternating pass by pass: every form sees the same box in the same state
        for k, f in passes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    us = {k: sorted(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}
    stats = {k: {"min": v[0], "median": v[len(v) // 2], "max": v[-1]} for k, v in us.items()}
    out = {"B": B, "lengths": lens, "rows": L, "N": N, "K": list(KS), "max_seq_len": MAX_SEQ_LEN,
           "mode": "forward + backward, eager, one device-event pair a pass", "block": _lib.JAGGED_BMM_BLOCK, "chunk": _lib.JAGGED_BMM_CHUNK,
           "warm_up_passes": WARM, "timed_passes": RUNS, "us_per_pass": stats, "peak_bytes": peaks, "max_abs_difference_fused_to_literal": diff,
           "fused_median_below_literal": {f"K{K}": stats[f"K{K}_fused"]["median"] < stats[f"K{K}_literal"]["median"] for K in KS},
           "fused_range_wholly_below_literal": {f"K{K}": stats[f"K{K}_fused"]["max"] < stats[f"K{K}_literal"]["min"] for K in KS}}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
