"""The cross network of dcn_v1 (csrc/cross_net.hip) against the reference's literal loop (interaction.FUSED_CROSS = False) on
the same box in the same run: `Cross` forward + backward alone at B = 8192 for (D, L) = (429, 3) (a Criteo-shaped group:
26 x 16 + 13) and (256, 3), and one train step of tests/golden/dcn_mini.config at B = 8192.

    python scripts/profile_cross_net.py time [out.json]      device events, fused and literal alternating, spread over rounds
    python scripts/profile_cross_net.py trace fused|literal  ITERS forward + backward passes of every shape and nothing else:
                                                             run under `rocprofv3 --kernel-trace --stats`, one pass per form;
                                                             the sum of the kernel times / ITERS is the device time of a pass

Bytes a fused launch has to move, from the shapes: forward 2 B D 4 (x in, y out) + B L 4 (s); backward 3 B D 4 (g, x in, dx
out) + B L 4 + G ((L + 1) D + L) 4 of partial sums (G = min(512, B / 4) workgroups), which the finishing launch reads again."""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, interaction  # noqa: E402
from torcheasyrec_amd.interaction import Cross  # noqa: E402

B = 8192
SHAPES = [(429, 3), (256, 3)]
ITERS = 50


def bytes_moved(D, L):
    G = min(512, (B + 3) // 4)
    parts = G * ((L + 1) * D + L) * 4
    return {"fwd": 2 * B * D * 4 + B * L * 4, "bwd_main": 3 * B * D * 4 + B * L * 4 + parts, "bwd_finish": parts + 2 * L * D * 4,
            "fwd_floor": 2 * B * D * 4, "bwd_floor": 3 * B * D * 4}


def cross_pass(dev, D, L):
    torch.manual_seed(0)
    m = Cross(D, L).to(dev)
    with torch.no_grad():
        for b in m.b:
            b.normal_(0, 0.1)
    x = (0.5 * torch.randn(B, D, device=dev)).requires_grad_(True)
    gy = torch.randn(B, D, device=dev)

    def run():
        x.grad = None
        for p in m.parameters():
            p.grad = None
        m(x).backward(gy)

    return run


def dcn_step(dev):
    from examples.train_from_config import synthetic_batches
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.dense import FusedDenseAdam
    from torcheasyrec_amd.embedding_group import _backward_of_losses, _losses_and_predictions
    from torcheasyrec_amd.rank_model import build_rank_model

    spec = load_pipeline_spec(open(os.path.join(ROOT, "tests", "golden", "dcn_mini.config")).read())
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
    interaction.FUSED_CROSS = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {f"cross D={D} L={L}": cross_pass(dev, D, L) for D, L in SHAPES}
    if mode == "trace":
        interaction.FUSED_CROSS = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    work["dcn_mini step"] = dcn_step(dev)
    out = {"B": B, "iters_per_round": ITERS, "bytes": {f"D={D} L={L}": bytes_moved(D, L) for D, L in SHAPES}, "us_per_pass": {}}
    for name, run in work.items():
        for fused in (True, False):  # warm-up of both forms
            timed(run, fused, 10)
        rounds = {"fused": [], "literal": []}
        for _ in range(6):  # alternating: both forms see the same box
            rounds["fused"].append(timed(run, True, ITERS))
            rounds["literal"].append(timed(run, False, ITERS))
        out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
        print(name, json.dumps(out["us_per_pass"][name]))
    interaction.FUSED_CROSS = True
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
