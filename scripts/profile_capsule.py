"""MIND's capsule layer (csrc/capsule_routing.hip) and label-aware attention (csrc/label_attention.hip) against the reference's
literal forms -- the pad to [B, S, L], the [B, S, H] low capsules and their normalized copy, [B, S, K] logits and six ops a
routing round (capsule.FUSED_CAPSULE = False); einsum, minimum, softmax, multiply, sum (match.FUSED_LABEL_ATTENTION = False) --
on the same box in the same process, forward + backward on the same inputs:

    capsule     B = 8192 histories of 0 .. 50 clicks (uniform), S = 50, L = H = 64, K = 5, 3 iterations, the default routing
                settings (scale 20, stddev 1, pow 1), given logits [N, K]; the rows and the bilinear matrix get their gradient
    attention   B = 8192, K = 5 (the capsule masks of the same lengths), D = 64, simi_pow 10, 1024 more item rows behind the
                positives; the interests and the items get their gradient

    python scripts/profile_capsule.py time [out.json]       one device-event pair per pass, RUNS passes per form after WARM warm-up
                                                            passes of each, fused and literal ALTERNATING pass by pass with nothing
                                                            in between (the device stays busy); the median per form, and
                                                            torch.cuda.max_memory_allocated of one forward + backward per form
                                                            above what the inputs take
    python scripts/profile_capsule.py trace fused|literal   ITERS forward + backward passes of both ops and nothing else: run under
                                                            `rocprofv3 --kernel-trace --stats`, one run per form (no counters in
                                                            the same run); launches / ITERS is the launch count of a pass"""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, capsule, match  # noqa: E402

B, S, L, H, K, ITERS_ROUTING, D, NEG, SIMI_POW = 8192, 50, 64, 64, 5, 3, 64, 1024, 10.0
WARM, RUNS, ITERS = 10, 60, 20
CFG = capsule.CapsuleConfig(max_k=K, max_seq_len=S, high_dim=H, num_iters=ITERS_ROUTING)


def lengths():
    return torch.randint(0, S + 1, (B,), generator=torch.Generator().manual_seed(0))


def capsule_pass(dev):
    torch.manual_seed(0)
    lens = lengths()
    offsets = torch.cat([lens.new_zeros(1), lens.cumsum(0)]).to(dev)
    n = int(offsets[-1])
    x = (0.5 * torch.randn(n, L, device=dev)).requires_grad_(True)
    w = torch.randn(L, H, device=dev).requires_grad_(True)
    logits0 = torch.randn(n, K, device=dev)
    g = torch.randn(B, K, H, device=dev)
    assert capsule.capsule_ok(x, offsets, w, CFG, logits0)

    def run():
        high, _ = capsule.capsule_routing(x, offsets, w, CFG, logits0)
        return torch.autograd.grad(high, [x, w], g)

    return run


def attention_pass(dev):
    torch.manual_seed(1)
    lens = lengths()
    kb = torch.stack([(2 ** j < lens) for j in range(K)], dim=1).sum(1).clamp(min=1)
    mask = (torch.arange(K)[None, :] < kb[:, None]).to(dev)
    interests = torch.nn.functional.normalize(torch.randn(B, K, D, device=dev), dim=-1).requires_grad_(True)
    item = torch.nn.functional.normalize(torch.randn(B + NEG, D, device=dev), dim=-1).requires_grad_(True)
    g = torch.randn(B, D, device=dev)
    assert match.label_attention_ok(interests, item, mask, SIMI_POW)

    def run():
        return torch.autograd.grad(match.label_attention(interests, item, mask, SIMI_POW), [interests, item], g)

    return run


def switch(fused):
    capsule.FUSED_CAPSULE = match.FUSED_LABEL_ATTENTION = fused


def one(run, fused):
    switch(fused)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    return a, b


def peak_bytes(run, fused):
    switch(fused)
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
    defaults = (capsule.FUSED_CAPSULE, match.FUSED_LABEL_ATTENTION)
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {"capsule": capsule_pass(dev), "attention": attention_pass(dev)}
    if mode == "trace":
        switch(sys.argv[2] == "fused")
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    out = {"B": B, "S": S, "L": L, "H": H, "K": K, "num_iters": ITERS_ROUTING, "D": D, "simi_pow": SIMI_POW, "warm_up_passes": WARM,
           "timed_passes": RUNS, "padded_low_capsule_bytes": B * S * H * 4, "us_per_pass": {}, "peak_bytes": {}}
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
    capsule.FUSED_CAPSULE, match.FUSED_LABEL_ATTENTION = defaults
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
