"""MaskNet's row kernels (csrc/ln_mask.hip) against the reference's literal loop (masknet.FUSED_MASKNET = False) on the same box
in the same run: `MaskNetModule` forward + backward alone at B = 8192, D = 429 (a Criteo-shaped group: 26 x 16 + 13), three
parallel blocks, hidden_dim 512, reduction_ratio 1, and one train step of tests/golden/masknet_mini.config at B = 8192.

    python scripts/profile_masknet.py time [out.json]        device events, fused and literal alternating, spread over rounds
    python scripts/profile_masknet.py trace fused|literal    ITERS forward + backward passes of the module and nothing else:
                                                             run under `rocprofv3 --kernel-trace --stats`, one pass per form
    python scripts/profile_masknet.py split fused.csv literal.csv [out.json]
                                                             the two passes' per-kernel CSVs (scripts/rocpd_stats.py) as device
                                                             time and launches per pass, GEMM and non-GEMM apart

Bytes the non-GEMM work has to move, from the shapes (n blocks, H = hidden_dim, 4-byte floats; `bytes_moved`).  Fused: the first
launch reads x and n masks and writes n products; the second reads n z and writes the [B, n H] concat; the backward reads and
writes the same tensors' gradients once more plus x / z again, and G rows of partial sums which the finishing launch reads
back.  Literal: LN(x) is written and read back by every block, every `LN -> ReLU` is two passes, the concat one more, and
autograd's backward of each is a pass of its own with [B, D] temporaries between them."""
import csv
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, masknet  # noqa: E402
from torcheasyrec_amd.masknet import MaskNetModule  # noqa: E402

B, D, N, H, RATIO = 8192, 429, 3, 512, 1.0
ITERS = 50
# kernels of the set-up (random inputs, parameter initialisation, copies), not of a pass
SETUP = ("distribution_", "copyBuffer", "fillBuffer", "FillFunctor", "uniform_", "normal_")
GEMM = ("Cijk_", "gemm", "Gemm", "GEMM")


def bytes_moved():
    G = min(512, (B + 3) // 4)
    f = 4
    fused = {"fwd_ln_mask": (1 + 2 * N) * B * D * f, "fwd_ln_relu_concat": 2 * N * B * H * f,
             "bwd_ln_relu_concat": 3 * N * B * H * f + 2 * N * G * 2 * H * f,
             "bwd_ln_mask": (1 + 2 * N) * B * D * f + (1 + N) * B * D * f + 2 * G * 2 * D * f}
    # literal forward: LN(x) (read x, write), per block a multiply (read 2, write 1), LN (2), ReLU (2), then the concat (2 n B H)
    lit_f = 2 * B * D * f + N * 3 * B * D * f + N * 4 * B * H * f + 2 * N * B * H * f
    # literal backward: concat split (2), ReLU (3), LN (read g, z, write gz: 3, + its two column sums), multiply (read g, a, b, write 2: 5),
    # n - 1 additions into d LN(x) (3 each), LN (3)
    lit_b = N * (2 + 3 + 3) * B * H * f + N * 5 * B * D * f + (N - 1) * 3 * B * D * f + 3 * B * D * f
    return {"fused": fused, "fused_total": sum(fused.values()), "literal_fwd": lit_f, "literal_bwd": lit_b, "literal_total": lit_f + lit_b}


def module_pass(dev):
    torch.manual_seed(0)
    m = MaskNetModule(D, N, {"hidden_dim": H, "reduction_ratio": RATIO}, use_parallel=True).to(dev)
    with torch.no_grad():
        for l in m.modules():
            if isinstance(l, torch.nn.LayerNorm):
                l.weight.normal_(1.0, 0.3)
                l.bias.normal_(0.0, 0.3)
    x = torch.randn(B, D, device=dev).requires_grad_(True)
    gy = torch.randn(B, N * H, device=dev)

    def run():
        x.grad = None
        for p in m.parameters():
            p.grad = None
        m(x).backward(gy)

    return run


def mini_step(dev):
    from examples.train_from_config import synthetic_batches
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import _backward_of_losses, _losses_and_predictions
    from torcheasyrec_amd.rank_model import build_rank_model

    spec = load_pipeline_spec(open(os.path.join(ROOT, "tests", "golden", "masknet_mini.config")).read())
    torch.manual_seed(0)
    model = build_rank_model(spec, device=dev)
    opt = FusedDenseAdam(list(model.dense_parameters()), lr=spec.dense_lr)
    batch = next(synthetic_batches(spec, B, B, seed=1)).to(dev)

    def run():
        opt.zero_grad(set_to_none=True)
        losses, _ = _losses_and_predictions(model, model.loss, batch)
        _backward_of_losses(losses)
        opt.step()

    return run


def timed(run, fused, n):
    masknet.FUSED_MASKNET = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def split(path):
    """per pass: device time and launches of the GEMM kernels and of everything else (set-up kernels left out)"""
    out = {"gemm_us": 0.0, "gemm_launches": 0.0, "other_us": 0.0, "other_launches": 0.0, "row_kernels_us": 0.0, "left_out": []}
    for r in csv.DictReader(open(path)):
        name, calls, total = r["kernel"], int(r["calls"]), float(r["total_us"])
        if any(s in name for s in SETUP) or calls < ITERS:
            out["left_out"].append(name[:60])
            continue
        kind = "gemm" if any(s in name for s in GEMM) else "other"
        out[f"{kind}_us"] += total / ITERS
        out[f"{kind}_launches"] += calls / ITERS
        if "tzr_ln_mask" in name:
            out["row_kernels_us"] += total / ITERS
    out["total_us"] = out["gemm_us"] + out["other_us"]
    out["launches"] = out["gemm_launches"] + out["other_launches"]
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "split":
        out = {"B": B, "D": D, "n": N, "hidden_dim": H, "iters": ITERS, "fused": split(sys.argv[2]), "literal": split(sys.argv[3]),
               "bytes": bytes_moved()}
        print(json.dumps(out, indent=1))
        if len(sys.argv) > 4:
            with open(sys.argv[4], "w") as f:
                json.dump(out, f, indent=1)
        return
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {f"masknet B={B} D={D} n={N} H={H}": module_pass(dev)}
    if mode == "trace":
        masknet.FUSED_MASKNET = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    work["masknet_mini step"] = mini_step(dev)
    out = {"B": B, "iters_per_round": ITERS, "bytes": bytes_moved(), "us_per_pass": {}}
    for name, run in work.items():
        for fused in (True, False):  # warm-up of both forms
            timed(run, fused, 10)
        rounds = {"fused": [], "literal": []}
        for _ in range(6):  # alternating: both forms see the same box
            rounds["fused"].append(timed(run, True, ITERS))
            rounds["literal"].append(timed(run, False, ITERS))
        out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
        print(name, json.dumps(out["us_per_pass"][name]))
    masknet.FUSED_MASKNET = True
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
