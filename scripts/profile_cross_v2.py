"""The low-rank cross network of dcn_v2 (csrc/cross_v2.hip) against the reference's literal loop (interaction.FUSED_CROSS_V2 =
False) on the same box in the same run: `CrossV2` forward + backward alone at B = 8192, r = 32, L = 3 for D = 429 (a
Criteo-shaped group: 26 x 16 + 13) and D = 256, and one train step of tests/golden/dcn_v2_mini.config at B = 8192.

    python scripts/profile_cross_v2.py time [out.json]      device events, fused and literal alternating, spread over rounds
    python scripts/profile_cross_v2.py trace fused|literal  ITERS forward + backward passes of every shape and nothing else:
                                                            run under `rocprofv3 --kernel-trace --stats`, one pass per form (no
                                                            counters in the same run); the sum of the kernel times / ITERS is
                                                            the device time of a pass

Bytes a fused pass has to move, from the shapes: forward 2 B D 4 (x in, y out) + (L - 1) B D 4 + L B r 4 (the saved x_l and
t_l); backward row pass 3 B D 4 (g, x in, dx out) + L B r 4 (t_l in) + L B (D + r) 4 (dy_l, dt_l out); weight-gradient pass
2 L B (D + r) 4 (dy_l, t_l, dt_l, x_l in).  The parameters (3 L D r floats at most) stay in L2."""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, interaction  # noqa: E402
from torcheasyrec_amd.interaction import CrossV2  # noqa: E402

B = 8192
R = 32
SHAPES = [(429, 3), (256, 3)]
ITERS = 50


def bytes_moved(D, L):
    rows, ws = B * D * 4, L * B * (D + R) * 4
    return {"fwd": 2 * rows + (L - 1) * rows + L * B * R * 4, "bwd_rows": 3 * rows + L * B * R * 4 + ws, "bwd_wgrad": 2 * ws,
            "fwd_floor": 2 * rows, "bwd_floor": 3 * rows}


def cross_pass(dev, D, L):
    torch.manual_seed(0)
    m = CrossV2(D, L, R).to(dev)
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

    spec = load_pipeline_spec(open(os.path.join(ROOT, "tests", "golden", "dcn_v2_mini.config")).read())
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
    interaction.FUSED_CROSS_V2 = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = interaction.FUSED_CROSS_V2
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {f"cross_v2 D={D} r={R} L={L}": cross_pass(dev, D, L) for D, L in SHAPES}
    if mode == "trace":
        interaction.FUSED_CROSS_V2 = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    work["dcn_v2_mini step"] = dcn_step(dev)
    out = {"B": B, "r": R, "iters_per_round": ITERS, "bytes": {f"D={D} L={L}": bytes_moved(D, L) for D, L in SHAPES}, "us_per_pass": {}}
    for name, run in work.items():
        for fused in (True, False):  # warm-up of both forms
            timed(run, fused, 10)
        rounds = {"fused": [], "literal": []}
        for _ in range(6):  # alternating: both forms see the same box
            rounds["fused"].append(timed(run, True, ITERS))
            rounds["literal"].append(timed(run, False, ITERS))
        out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
        print(name, json.dumps(out["us_per_pass"][name]))
    interaction.FUSED_CROSS_V2 = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
