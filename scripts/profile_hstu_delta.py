"""HSTU's delta attention (csrc/hstu_delta.hip, hstu.FUSED_HSTU_DELTA) at one serving step, forward only, on the same box in the
same process on the same inputs:

    B = 8 samples with 0 .. 4096 cached rows (uniform), delta = 32 new rows a sample, all of them targets, H = 4, Da = Dv = 128, a
    contextual prefix of 4 rows, max_seq_len 4096 + 32, alpha = 128^-1/2.  The cache is a buffer of its own; the delta rows' q, k, v
    are column slices of one uvqk matrix.

    (a) fused     hstu.delta_hstu_mha in its two-segment form on the kernel (cache and delta rows read where they lie)
    (b) literal   hstu.delta_hstu_mha_literal in its two-segment form: the concat of cache and delta rows, then the padded torch form
    (c) full      what a caller without the delta path does: the concat, hstu.hstu_mha (fused, csrc/hstu_attention.hip) over the full
                  sequences with arbitrary q in front of the delta rows, then the slice of the delta rows

    python scripts/profile_hstu_delta.py time [out.json] [CHUNK=lib.so ..]   CALLS calls between one device-event pair, RUNS pairs per
                                                          form after WARM warm-up rounds, the forms ALTERNATING; the median, minimum
                                                          and maximum per call and form, the peak memory of one call, (a) against (b).
                                                          Every `CHUNK=lib.so` adds form (a) on a library built with that
                                                          TZR_HSTU_DELTA_CHUNK (the candidates of the chunk length)
    python scripts/profile_hstu_delta.py build DIR CHUNK ..                  build those libraries (needs hipcc and a built tree)
    python scripts/profile_hstu_delta.py trace fused|literal|full            ITERS calls and nothing else: run under `rocprofv3
                                                                             --kernel-trace --stats`, one run per form"""
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _build, _lib, hstu  # noqa: E402

B, NC, DELTA, H, DA, DV, CONTEXTUAL = 8, int(os.environ.get("HSTU_DELTA_NC", 4096)), 32, 4, 128, 128, 4  # (HSTU_DELTA_NC: a second cache bound)
WARM, RUNS, CALLS, ITERS = 3, 30, 10, 5


def build_variant(out_dir, chunk):
    """libtzrec_hip.so with csrc/hstu_delta.hip compiled at another TZR_HSTU_DELTA_CHUNK (every other object as built)"""
    os.makedirs(out_dir, exist_ok=True)
    objs = _build.build_objects(_build.shutil.which("hipcc") or "/opt/rocm/bin/hipcc", os.path.join(os.path.dirname(_build.OUT), "_obj"))
    obj, out = os.path.join(out_dir, f"hstu_delta_{chunk}.o"), os.path.join(out_dir, f"libtzrec_hip_chunk{chunk}.so")
    hipcc = _build.shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, f"--offload-arch={_build.ARCH}", *_build.FLAGS, f"-DTZR_HSTU_DELTA_CHUNK={chunk}", "-c",
                           os.path.join(_build.CSRC, "hstu_delta.hip"), "-o", obj])
    subprocess.check_call([hipcc, f"--offload-arch={_build.ARCH}", "-fPIC", "-shared", *[o for o in objs if not o.endswith("hstu_delta.hip.o")], obj, "-o", out])
    return out


def make_step(dev):
    gen = torch.Generator().manual_seed(0)
    n1 = torch.randint(0, NC + 1, (B,), generator=gen)
    off = torch.cat([n1.new_zeros(1), n1.cumsum(0)]).to(dev)
    Lc, Ld, N = int(n1.sum()), B * DELTA, NC + DELTA
    targets = torch.full((B,), DELTA, dtype=torch.int64, device=dev)
    torch.manual_seed(0)
    k_cache, v_cache = torch.randn(Lc, H, DA, device=dev), torch.randn(Lc, H, DV, device=dev)
    uvqk = torch.randn(Ld, (2 * DV + 2 * DA) * H, device=dev)
    _, v, q, k = torch.split(uvqk, [DV * H, DV * H, DA * H, DA * H], dim=1)
    dq, dk, dv = q.view(Ld, H, DA), k.view(Ld, H, DA), v.view(Ld, H, DV)
    q_front = torch.randn(Lc, H * DA, device=dev)  # (form (c): the rows in front of the delta rows need some q)
    kw = dict(num_targets=targets, contextual_seq_len=CONTEXTUAL)

    def fused():
        return hstu.delta_hstu_mha(N, DA ** -0.5, dq, k_cache, v_cache, off, delta_k=dk, delta_v=dv, **kw)

    def literal():
        return hstu.delta_hstu_mha_literal(N, DA ** -0.5, dq, k_cache, v_cache, off, delta_k=dk, delta_v=dv, **kw)

    def full():
        fk, fo = hstu.concat_cache_delta(k_cache.view(Lc, -1), dk.reshape(Ld, -1), off, DELTA)
        fv, _ = hstu.concat_cache_delta(v_cache.view(Lc, -1), dv.reshape(Ld, -1), off, DELTA)
        fq, _ = hstu.concat_cache_delta(q_front, dq.reshape(Ld, -1), off, DELTA)
        out = hstu.hstu_mha(N, DA ** -0.5, fq.view(-1, H, DA), fk.view(-1, H, DA), fv.view(-1, H, DV), fo, **kw)
        rows = (fo[1:].view(-1, 1) - DELTA + torch.arange(DELTA, device=dev)).view(-1)
        return out[rows]

    return {"fused": fused, "literal": literal, "full": full}, n1.tolist()


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
    if mode == "build":
        for chunk in sys.argv[3:]:
            print(build_variant(sys.argv[2], int(chunk)))
        return
    native = _build.build()
    _lib.use_library(native)
    assert _lib.backend().startswith("hip")
    hstu.FUSED_HSTU_DELTA = hstu.FUSED_HSTU_MHA = True
    step, n1 = make_step(torch.device("cuda", 0))
    if mode == "trace":
        for _ in range(ITERS):
            step[sys.argv[2]]()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} calls")
        return
    before = hstu._HstuDeltaFn.calls
    got, lit, full = step["fused"](), step["literal"](), step["full"]()
    assert hstu._HstuDeltaFn.calls == before + 1
    forms, libs = {}, {"fused": native, "literal": native, "full": native}
    for name, f in step.items():
        forms[name] = f
    for spec in sys.argv[3:]:  # the chunk-length candidates: form (a) on another library
        chunk, path = spec.split("=")
        forms[f"fused_chunk{chunk}"], libs[f"fused_chunk{chunk}"] = step["fused"], os.path.abspath(path)
    peaks = {k: peak_bytes(step[k]) for k in step}
    equal = {}
    for k in forms:
        _lib.use_library(libs[k])
        for _ in range(WARM):
            out = forms[k]()
        equal[k] = float((out - lit).abs().max())
    torch.cuda.synchronize()
    ev = {k: [] for k in forms}
    for _ in range(RUNS):  # alternating round by round: every form sees the same box in the same state
        for k, f in forms.items():
            _lib.use_library(libs[k])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    us = {k: sorted(a.elapsed_time(b) * 1e3 / CALLS for a, b in v) for k, v in ev.items()}
    stats = {k: {"min": v[0], "median": v[len(v) // 2], "max": v[-1]} for k, v in us.items()}
    out = {"B": B, "cached_rows": n1, "delta": DELTA, "num_targets": DELTA, "H": H, "Da": DA, "Dv": DV, "contextual_seq_len": CONTEXTUAL, "max_seq_len": NC + DELTA,
           "mode": "forward only, eager; (a) fused two-segment, (b) literal with its concat, (c) concat + fused hstu_mha over the full rows + slice",
           "chunk_of_the_shipped_library": _lib.HSTU_DELTA_CHUNK, "warm_up_rounds": WARM, "timed_rounds": RUNS, "calls_per_round": CALLS, "us_per_call": stats,
           "peak_bytes": peaks, "max_abs_difference_to_literal": equal, "max_abs_full_to_literal": float((full - lit).abs().max()),
           "fused_range_wholly_below_literal": stats["fused"]["max"] < stats["literal"]["min"]}
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
