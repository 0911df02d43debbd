"""The gate-and-scale step of PEPNet (csrc/gate_scale.hip) against the reference's literal form -- bias adds, ReLU, sigmoid, scale
and multiply as torch ops (personalized_net.FUSED_GATE_SCALE = False) -- on the same box in the same run, forward + backward at
B = 8192, at the shape of the reference's example (examples/pepnet_taobao.config): main embedding 256 wide, uia 208, two tasks,
ppnet_hidden_units [512, 256]:

    H = 512, N = 2   (the first PPNet level)
    H = 256, N = 2   (the second)

each as the gate-and-scale step alone (the GEMM outputs z and g given, the biases parameters) and as the whole `PPNet` (the
three GEMMs per task and level included).

    python scripts/profile_gate_scale.py time [out.json]      device events, fused and literal alternating, spread over rounds
    python scripts/profile_gate_scale.py trace fused|literal  ITERS forward + backward passes of the gate-and-scale step of both
                                                               levels and nothing else: run under `rocprofv3 --kernel-trace
                                                               --stats`, one pass per form (no counters in the same run);
                                                               launches / ITERS and the sum of the kernel times / ITERS are
                                                               the launch count and device time of a pass

Bytes a fused pass has to move, from the shapes: forward 3 N B H 4 (z, g in, out out); backward 5 N B H 4 (dout, z, g in; dz, dg
out); the biases and the partial sums are noise beside them."""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, personalized_net  # noqa: E402
from torcheasyrec_amd.personalized_net import PPNet  # noqa: E402

B = 8192
MAIN, UIA, TASKS, HIDDEN = 256, 208, 2, [512, 256]
GAMMA = 2.0
ITERS = 50


def bytes_moved(H, N):
    return {"fwd": 3 * N * B * H * 4, "bwd": 5 * N * B * H * 4}


def step_pass(dev, H, N):
    """PPNet.forward's step behind the GEMMs of one level, the GEMM outputs given"""
    from torcheasyrec_amd.gate_ops import gate_scale, gate_scale_ok

    torch.manual_seed(0)
    zs = [torch.randn(B, H, device=dev).requires_grad_(True) for _ in range(N)]
    gs = [torch.randn(B, H, device=dev).requires_grad_(True) for _ in range(N)]
    bzs = [(0.1 * torch.randn(H, device=dev)).requires_grad_(True) for _ in range(N)]
    bgs = [(0.1 * torch.randn(H, device=dev)).requires_grad_(True) for _ in range(N)]
    gouts = [torch.randn(B, H, device=dev) for _ in range(N)]
    assert gate_scale_ok(zs, gs, bzs, bgs)

    def run():
        if personalized_net.FUSED_GATE_SCALE:
            outs = gate_scale(zs, bzs, gs, bgs, GAMMA, relu=True)
        else:
            outs = [torch.relu(z + bz) * (GAMMA * torch.sigmoid(g + bg)) for z, bz, g, bg in zip(zs, bzs, gs, bgs)]
        torch.autograd.grad(outs, zs + bzs + gs + bgs, gouts)

    return run


def ppnet_pass(dev):
    torch.manual_seed(0)
    net = PPNet(MAIN, UIA, TASKS, HIDDEN, gamma=GAMMA).to(dev)
    x = (0.5 * torch.randn(B, MAIN, device=dev)).requires_grad_(True)
    uia = (0.5 * torch.randn(B, UIA, device=dev)).requires_grad_(True)
    gouts = [torch.randn(B, HIDDEN[-1], device=dev) for _ in range(TASKS)]

    def run():
        for p in net.parameters():
            p.grad = None
        x.grad, uia.grad = None, None
        torch.autograd.backward(net(x, uia), gouts)

    return run


def timed(run, fused, n):
    personalized_net.FUSED_GATE_SCALE = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = personalized_net.FUSED_GATE_SCALE
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {f"step H={H} N={TASKS}": step_pass(dev, H, TASKS) for H in HIDDEN}
    if mode == "trace":
        personalized_net.FUSED_GATE_SCALE = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    work[f"PPNet main={MAIN} uia={UIA} T={TASKS} hidden={HIDDEN}"] = ppnet_pass(dev)
    out = {"B": B, "iters_per_round": ITERS, "bytes": {f"H={H} N={TASKS}": bytes_moved(H, TASKS) for H in HIDDEN}, "us_per_pass": {}}
    for name, run in work.items():
        for fused in (True, False):  # warm-up of both forms
            timed(run, fused, 10)
        rounds = {"fused": [], "literal": []}
        for _ in range(6):  # alternating: both forms see the same box
            rounds["fused"].append(timed(run, True, ITERS))
            rounds["literal"].append(timed(run, False, ITERS))
        out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
        print(name, json.dumps(out["us_per_pass"][name]), flush=True)
    personalized_net.FUSED_GATE_SCALE = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
