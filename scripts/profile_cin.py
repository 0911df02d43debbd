"""The compressed interaction network of xdeepfm (csrc/cin.hip) against the reference's literal loop (interaction.FUSED_CIN =
False) on the same box in the same run: `CIN` forward + backward alone at the Criteo-shaped wide group B = 8192, F = 26, D = 16,
cin_layer_size = [128, 128], and one train step of tests/golden/xdeepfm_mini.config at B = 8192.

    python scripts/profile_cin.py time [out.json]      device events, fused and literal alternating, spread over rounds
    python scripts/profile_cin.py trace fused|literal  ITERS forward + backward passes and nothing else: run under
                                                       `rocprofv3 --kernel-trace`, one pass per form, summarised by
                                                       scripts/rocpd_stats.py; the sum of the kernel times / ITERS is the
                                                       device time of a pass
    python scripts/profile_cin.py peak stats.csv [timings.json]
                                                       per kernel of a fused trace: its share of the pass's FLOPs over its device
                                                       time, as a fraction of the 157.3 TF fp32 MFMA peak

FLOPs of a pass, from the shapes: forward 2 B D sum_i O_i H_i F; backward twice that, half in the weight-gradient kernel and
half in the input-gradient kernel."""
import csv
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

B, F, D, LAYERS = 8192, 26, 16, [128, 128]
ITERS = 20
PEAK_TF = 157.3


def flops_fwd():
    hs = [F] + LAYERS[:-1]
    return 2 * B * D * sum(o * h * F for o, h in zip(LAYERS, hs))


def cin_pass(dev):
    from torcheasyrec_amd.interaction import CIN

    torch.manual_seed(0)
    m = CIN(F, LAYERS).to(dev)
    x = (0.5 * torch.randn(B, F, D, device=dev)).requires_grad_(True)
    gy = torch.randn(B, sum(LAYERS), device=dev)

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

    spec = load_pipeline_spec(open(os.path.join(ROOT, "tests", "golden", "xdeepfm_mini.config")).read())
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
    from torcheasyrec_amd import interaction

    interaction.FUSED_CIN = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def peak(stats_csv, out_json=None):
    """rows of scripts/rocpd_stats.py's csv of a `trace fused` pass -> us per pass and fraction of peak per kernel of csrc/cin.hip"""
    share = {"cin_fwd_kernel": 1.0, "cin_bwd_w_kernel": 1.0, "cin_bwd_x_kernel": 1.0}  # each of the three does one forward's FLOPs per pass
    res = {}
    for row in csv.DictReader(open(stats_csv)):
        name = next((k for k in list(share) + ["cin_bwd_finish_kernel"] if k in row["kernel"]), None)
        if name is None:
            continue
        us = float(row["total_us"]) / ITERS
        res[name] = {"us_per_pass": us, "launches_per_pass": int(row["calls"]) / ITERS}
        if name in share:
            res[name]["fraction_of_fp32_mfma_peak"] = share[name] * flops_fwd() / (us * 1e-6) / (PEAK_TF * 1e12)
    print(json.dumps(res, indent=1))
    if out_json:
        doc = json.load(open(out_json)) if os.path.exists(out_json) else {}
        doc["kernels"] = res
        with open(out_json, "w") as f:
            json.dump(doc, f, indent=1)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "peak":
        return peak(*sys.argv[2:4])
    from torcheasyrec_amd import _lib, interaction

    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {f"cin B={B} F={F} D={D} {LAYERS}": cin_pass(dev)}
    if mode == "trace":
        interaction.FUSED_CIN = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    work["xdeepfm_mini step"] = mini_step(dev)
    out = {"B": B, "F": F, "D": D, "cin_layer_size": LAYERS, "iters_per_round": ITERS, "flops_forward": flops_fwd(),
           "flops_backward": 2 * flops_fwd(), "launches": {"fused": {"forward": 1, "backward": 2 * len(LAYERS) + 1}}, "us_per_pass": {}}
    for name, run in work.items():
        for fused in (True, False):  # warm-up of both forms
            timed(run, fused, 3)
        rounds = {"fused": [], "literal": []}
        for _ in range(5):  # alternating: both forms see the same box
            rounds["fused"].append(timed(run, True, ITERS))
            rounds["literal"].append(timed(run, False, ITERS))
        out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
        print(name, json.dumps(out["us_per_pass"][name]))
    interaction.FUSED_CIN = True
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
