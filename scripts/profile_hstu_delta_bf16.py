"""HSTU's delta attention in bf16 (csrc/hstu_delta_bf16.hip, hstu.FUSED_HSTU_DELTA_BF16) at the serving step of
scripts/profile_hstu_delta.py (its shape, seeds and method), forward only, on the same box in the same process:

    (a) bf16_fused     hstu.delta_hstu_mha on bf16 operands in its two-segment form on the kernel (a bf16 cache, bf16 uvqk slices)
    (b) bf16_literal   hstu.delta_hstu_mha_literal on the same bf16 operands: the concat, then the padded torch form
    (c) fp32_fused     hstu.delta_hstu_mha on the fp32 operands the bf16 ones were rounded from (csrc/hstu_delta.hip): reported, not gated on

    python scripts/profile_hstu_delta_bf16.py time [out.json]     CALLS calls between one device-event pair, RUNS pairs per form after WARM
                                                                  warm-up rounds, the forms ALTERNATING; the median, minimum and maximum
                                                                  per call and form, the peak memory of one call, (a) against (b)
    python scripts/profile_hstu_delta_bf16.py trace FORM          ITERS calls and nothing else: run under `rocprofv3 --kernel-trace --stats`"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import profile_hstu_delta as base  # noqa: E402  (the shape, the rounds and peak_bytes)
from torcheasyrec_amd import _build, _lib, hstu  # noqa: E402

BF = torch.bfloat16


def make_step(dev):
    B, NC, DELTA, H, DA, DV = base.B, base.NC, base.DELTA, base.H, base.DA, base.DV
    gen = torch.Generator().manual_seed(0)
    n1 = torch.randint(0, NC + 1, (B,), generator=gen)
    off = torch.cat([n1.new_zeros(1), n1.cumsum(0)]).to(dev)
    Lc, Ld, N = int(n1.sum()), B * DELTA, NC + DELTA
    kw = dict(num_targets=torch.full((B,), DELTA, dtype=torch.int64, device=dev), contextual_seq_len=base.CONTEXTUAL)
    torch.manual_seed(0)
    k16, v16 = torch.randn(Lc, H, DA, device=dev).to(BF), torch.randn(Lc, H, DV, device=dev).to(BF)
    uvqk16 = torch.randn(Ld, (2 * DV + 2 * DA) * H, device=dev).to(BF)
    forms = {}
    for name, dtype, fn in (("bf16_fused", BF, hstu.delta_hstu_mha), ("bf16_literal", BF, hstu.delta_hstu_mha_literal), ("fp32_fused", torch.float32, hstu.delta_hstu_mha)):
        kc, vc, uvqk = k16.to(dtype), v16.to(dtype), uvqk16.to(dtype)  # (fp32: the same values widened)
        _, v, q, k = torch.split(uvqk, [DV * H, DV * H, DA * H, DA * H], dim=1)
        forms[name] = (lambda fn=fn, a=(q.view(Ld, H, DA), kc, vc, off), dk=k.view(Ld, H, DA), dv=v.view(Ld, H, DV):
                       fn(N, DA ** -0.5, *a, delta_k=dk, delta_v=dv, **kw))
    return forms, n1.tolist()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    _lib.use_library(_build.build())
    assert _lib.backend().startswith("hip")
    hstu.FUSED_HSTU_DELTA = hstu.FUSED_HSTU_DELTA_BF16 = True
    step, n1 = make_step(torch.device("cuda", 0))
    if mode == "trace":
        for _ in range(base.ITERS):
            step[sys.argv[2]]()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {base.ITERS} calls")
        return
    before = hstu._HstuDeltaFn.calls
    outs = {k: f() for k, f in step.items()}
    assert hstu._HstuDeltaFn.calls == before + 2 and outs["bf16_fused"].dtype == BF
    peaks = {k: base.peak_bytes(f) for k, f in step.items()}
    for _ in range(base.WARM):
        for f in step.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in step}
    for _ in range(base.RUNS):  # alternating round by round: every form sees the same box in the same state
        for k, f in step.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(base.CALLS):
                f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    us = {k: sorted(a.elapsed_time(b) * 1e3 / base.CALLS for a, b in v) for k, v in ev.items()}
    stats = {k: {"min": v[0], "median": v[len(v) // 2], "max": v[-1]} for k, v in us.items()}
    out = {"B": base.B, "cached_rows": n1, "delta": base.DELTA, "num_targets": base.DELTA, "H": base.H, "Da": base.DA, "Dv": base.DV,
           "contextual_seq_len": base.CONTEXTUAL, "max_seq_len": base.NC + base.DELTA,
           "mode": "forward only, eager, two-segment form; (a) bf16 fused, (b) bf16 literal with its concat, (c) fp32 fused on the same values",
           "chunk": _lib.HSTU_DELTA_CHUNK, "warm_up_rounds": base.WARM, "timed_rounds": base.RUNS, "calls_per_round": base.CALLS, "us_per_call": stats, "peak_bytes": peaks,
           "max_abs_difference_to_fp32_fused": {k: float((outs[k].float() - outs["fp32_fused"]).abs().max()) for k in ("bf16_fused", "bf16_literal")},
           "bf16_fused_range_wholly_below_bf16_literal": stats["bf16_fused"]["max"] < stats["bf16_literal"]["min"]}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
