"""HSTU's positional and timestamp encoder (csrc/hstu_position.hip, hstu.FUSED_HSTU_POSITION) at the recorded HSTU shape of
scripts/profile_hstu_attention.py (its lengths and seed): B = 16 samples of 0 .. 4096 rows, E = 512, P = 8192 position rows,
T = 2048 time buckets, 0 .. 8 targets a sample, a contextual prefix of 4, timestamps ascending within a sample with the targets'
equal to the request time.  One forward plus backward (out, then dx and both table gradients under a fixed g), four forms:

    fp32_fused / fp32_literal / bf16_fused / bf16_literal      the kernels against hstu's own literal form, per dtype

    python scripts/profile_hstu_position.py time [out.json]   RUNS device-event pairs a form after WARM warm-up passes, the forms
                                                               ALTERNATING pass by pass; median, minimum and maximum, the peak
                                                               memory of one pass, and per dtype whether the fused range lies
                                                               wholly below the literal one
    python scripts/profile_hstu_position.py trace FORM        ITERS passes and nothing else: run under `rocprofv3 --kernel-trace --stats`"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from torcheasyrec_amd import _build, _lib, hstu  # noqa: E402

B, N, E, P, T, CONTEXTUAL, MAX_TARGETS = 16, 4096, 512, 8192, 2048, 4, 8
WARM, RUNS, ITERS = 3, 40, 5


def make_passes(dev):
    gen = torch.Generator().manual_seed(0)
    lens = torch.randint(0, N + 1, (B,), generator=gen)
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)])
    targets = torch.minimum(torch.randint(0, MAX_TARGETS + 1, (B,), generator=gen), lens)
    L = int(lens.sum())
    # a sample's history: steps of 1 .. 3600 s up to the request time, which its targets share
    steps = torch.randint(1, 3601, (L,), generator=gen)
    tm = torch.zeros(L, dtype=torch.int64)
    for b in range(B):
        s, n, t = int(offsets[b]), int(lens[b]), int(targets[b])
        tm[s:s + n] = 1_700_000_000 + steps[s:s + n].cumsum(0)
        if t:
            tm[s + n - t:s + n] = tm[s + n - 1]
    torch.manual_seed(0)
    x32, g32 = torch.randn(L, E, device=dev), torch.randn(L, E, device=dev)
    pos32, ts32 = torch.randn(P, E, device=dev) * P ** -0.5, torch.randn(T + 1, E, device=dev) * T ** -0.5
    offsets, targets, tm = offsets.to(dev), targets.to(dev), tm.to(dev)
    passes = {}
    for dname, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x, pos, ts = (t.to(dt).requires_grad_(True) for t in (x32, pos32, ts32))
        g = g32.to(dt)
        for fname, fused in (("fused", True), ("literal", False)):
            def run(x=x, pos=pos, ts=ts, g=g, fused=fused):
                hstu.FUSED_HSTU_POSITION = fused
                out = hstu.add_timestamp_positional_embeddings(E ** 0.5, N, CONTEXTUAL, pos, ts, offsets, None, x, tm, targets, False)
                return (out, *torch.autograd.grad(out, [x, pos, ts], g))
            passes[f"{dname}_{fname}"] = run
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
    before = hstu._HstuPositionFn.calls
    outs = {k: f() for k, f in passes.items()}
    assert hstu._HstuPositionFn.calls == before + 2
    diff = {d: {k: float((a.float() - b.float()).abs().max()) for k, a, b in zip(("out", "dx", "dpos", "dts"), outs[d + "_fused"], outs[d + "_literal"])}
            for d in ("fp32", "bf16")}
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
    out = {"B": B, "lengths": lens, "rows": L, "E": E, "P": P, "T": T, "contextual_seq_len": CONTEXTUAL, "max_targets": MAX_TARGETS, "max_seq_len": N,
           "mode": "forward + backward, eager, one device-event pair a pass", "slab": _lib.HSTU_POS_SLAB, "warm_up_passes": WARM, "timed_passes": RUNS,
           "us_per_pass": stats, "peak_bytes": peaks, "max_abs_difference_fused_to_literal": diff,
           "fused_range_wholly_below_literal": {d: stats[d + "_fused"]["max"] < stats[d + "_literal"]["min"] for d in ("fp32", "bf16")}}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
