"""WuKong's FM front and mix kernels (csrc/wukong.hip) against the reference's literal forward (wukong.FUSED_WUKONG = False) on
the same box in the same run: one `WuKongLayer` forward + backward at the example's first layer, B = 8192, F = 27, D = 128,
Fl = Ff = 16, k = 24, feature_num_mlp [512].

    python scripts/profile_wukong.py time [out.json]        device events, fused and literal alternating, spread over rounds
    python scripts/profile_wukong.py trace fused|literal    ITERS forward + backward passes of the layer and nothing else:
                                                            run under `rocprofv3 --kernel-trace --stats`, one pass per form
    python scripts/profile_wukong.py split fused.csv literal.csv [out.json]
                                                            the two passes' per-kernel CSVs (scripts/rocpd_stats.py) as device
                                                            time and launches per pass, GEMM and non-GEMM apart

Bytes the non-GEMM work has to move, from the shapes (4-byte floats; `bytes_moved`).  Fused: the FM front reads x and writes
[B, F k] and the statistics; the mix reads x and fm and writes [B, Fo, D]; each backward reads its inputs and the output
gradient once more, writes an input gradient of x's size (the mix also fm's) and G rows of partial sums which the finishing
launch reads back; autograd adds the two gradients of x.  Literal: X^T W and X P are batched matmuls that write [B, D, k] and
[B, F, k]; the LayerNorm over F k is a pass; lcb and the residual projection each read x and write [B, D, Fl] / [B, D, Fo]
through their permutes; the concat, the add and the LayerNorm over D are a pass each over [B, Fo, D]; autograd's backward of
each is a pass of its own with a temporary between them."""
import csv
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, wukong  # noqa: E402
from torcheasyrec_amd.wukong import WuKongLayer  # noqa: E402

B, F, D, FL, FF, K, MLP = 8192, 27, 128, 16, 16, 24, [512]
FO = FL + FF
ITERS = 50
# kernels of the set-up (random inputs, parameter initialisation, copies), not of a pass
SETUP = ("distribution_", "copyBuffer", "fillBuffer", "FillFunctor", "uniform_", "normal_")
# by kernel name: the GEMMs both forms share (the FMB's MLP and feature_out_liner, three products each) and, in the literal form,
# the batched matmuls the kernels replace -- so the two forms' GEMM times differ by those, and the totals are the comparison
GEMM =("Cijk_", "gemm", "Gemm", "GEMM")


def bytes_moved():
    G = min(512, B)
    f = 4
    x, z, fm, y = B * F * D * f, B * F * K * f, B * FF * D * f, B * FO * D * f
    fused = {"fm_fwd": x + z + 2 * B * f, "mix_fwd": x + fm + y + 2 * B * FO * f,
             "fm_bwd": z + x + 2 * B * f + x + 2 * G * 3 * F * K * f,
             "mix_bwd": y + x + fm + 2 * B * FO * f + x + fm + 2 * G * (F * FO + F * FL + 2 * D) * f,
             "autograd_gx_add": 3 * x}
    # literal forward: X^T W (read x, write [B, D, k]), X P (read x and it, write z), LN (2 z); lcb and the projection (read x, write
    # [B, D, Fl] / [B, D, Fo]; the permutes are views until the concat / the add make them contiguous: 2 passes each), concat
    # (read fm and lcb, write y), add (3 y), LN (2 y)
    p = B * D * K * f
    lcb, res = B * FL * D * f, y
    lit_f = (x + p) + (x + p + z) + 2 * z + (x + lcb) + (x + res) + (fm + lcb + y) + 3 * y + 2 * y
    # literal backward: LN over D (read g, pre, write: 3 y), the add (y), the concat split (2 y), the two projections' input and
    # weight gradients (read g and x each: 2 (x + lcb) + 2 (x + res), write 2 x), LN over F k (3 z), X P (read gz, x, p; write gx and
    # gp: 2 x + 2 p + z), X^T W (read gp, x; write gx: 2 x + p), the additions of the four gradients of x (3 x each: 9 x)
    lit_b = 3 * y + y + 2 * y + 2 * (x + lcb) + 2 * (x + res) + 2 * x + 3 * z + (2 * x + 2 * p + z) + (2 * x + p) + 9 * x
    return {"fused": fused, "fused_total": sum(fused.values()), "literal_fwd": lit_f, "literal_bwd": lit_b, "literal_total": lit_f + lit_b}


def layer_pass(dev):
    torch.manual_seed(0)
    m = WuKongLayer(D, F, FL, FF, K, {"hidden_units": MLP}).to(dev)
    with torch.no_grad():
        for l in m.modules():
            if isinstance(l, torch.nn.LayerNorm):
                l.weight.normal_(1.0, 0.3)
                l.bias.normal_(0.0, 0.3)
    x = torch.randn(B, F, D, device=dev).requires_grad_(True)
    gy = torch.randn(B, FO, D, device=dev)

    def run():
        x.grad = None
        for p in m.parameters():
            p.grad = None
        m(x).backward(gy)

    return run


def timed(run, fused, n):
    wukong.FUSED_WUKONG = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def split(path):
    """per pass: device time and launches of the GEMM kernels and of everything else (set-up kernels left out)"""
    out = {"gemm_us": 0.0, "gemm_launches": 0.0, "other_us": 0.0, "other_launches": 0.0, "wukong_kernels_us": 0.0, "per_kernel": [],
           "left_out": []}
    for r in csv.DictReader(open(path)):
        name, calls, total = r["kernel"], int(r["calls"]), float(r["total_us"])
        if any(s in name for s in SETUP) or calls < ITERS:
            out["left_out"].append(name[:60])
            continue
        kind = "gemm" if any(s in name for s in GEMM) else "other"
        out[f"{kind}_us"] += total / ITERS
        out[f"{kind}_launches"] += calls / ITERS
        if "wk_" in name or "tzr_parts_sum_finish" in name:
            out["wukong_kernels_us"] += total / ITERS
        out["per_kernel"].append({"kernel": name[:80], "kind": kind, "launches": calls / ITERS, "us": total / ITERS})
    out["per_kernel"].sort(key=lambda r: -r["us"])
    out["total_us"] = out["gemm_us"] + out["other_us"]
    out["launches"] = out["gemm_launches"] + out["other_launches"]
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    shape = {"B": B, "F": F, "D": D, "lcb_feature_num": FL, "fmb_feature_num": FF, "compressed_feature_num": K, "feature_num_mlp": MLP}
    if mode == "split":
        out = dict(shape, iters=ITERS, fused=split(sys.argv[2]), literal=split(sys.argv[3]), bytes=bytes_moved())
        print(json.dumps(out, indent=1))
        if len(sys.argv) > 4:
            with open(sys.argv[4], "w") as f:
                json.dump(out, f, indent=1)
        return
    _lib.use_native()
    dev = torch.device("cuda", 0)
    name, run = f"wukong layer B={B} F={F} D={D} Fl={FL} Ff={FF} k={K} mlp={MLP}", layer_pass(dev)
    if mode == "trace":
        wukong.FUSED_WUKONG = sys.argv[2] == "fused"
        for _ in range(ITERS):
            run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of {name}")
        return
    out = dict(shape, iters_per_round=ITERS, bytes=bytes_moved(), us_per_pass={})
    for fused in (True, False):  # warm-up of both forms
        timed(run, fused, 10)
    rounds = {"fused": [], "literal": []}
    for _ in range(6):  # alternating: both forms see the same box
        rounds["fused"].append(timed(run, True, ITERS))
        rounds["literal"].append(timed(run, False, ITERS))
    out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
    wukong.FUSED_WUKONG = True
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
