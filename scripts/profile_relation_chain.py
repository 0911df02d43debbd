"""The relation towers of DBMTL (csrc/relation_chain.hip) against the reference's literal form -- per tower a torch.cat and the
relation MLP, layer by layer (rank_model.FUSED_RELATION_CHAIN = False; the MLP is this package's, with its Linear + bias + ReLU
epilogue) -- on the same box in the same run, forward + backward at B = 8192, on the same weights, at two shapes:

    taobao   the reference's example (examples/dbmtl_taobao_seq.config): ctr and cvr end 64 wide, cvr's relation MLP is
             [64 | 64] -> [64]
    chain4   four towers 64 wide; b reads a, c reads a and b, d reads b and c; relation MLPs [64, 32], [64, 32], [32, 16]

The towers' own outputs are given (leaves); every input and every relation parameter gets its gradient.

    python scripts/profile_relation_chain.py time [out.json]      device events, fused and literal alternating, spread over rounds
    python scripts/profile_relation_chain.py trace fused|literal  ITERS forward + backward passes of both shapes and nothing else:
                                                                   run under `rocprofv3 --kernel-trace --stats`, one pass per
                                                                   form (no counters in the same run); launches / ITERS and the
                                                                   sum of the kernel times / ITERS are the launch count and
                                                                   device time of a pass"""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib, rank_model  # noqa: E402
from torcheasyrec_amd.dlrm import MLP  # noqa: E402

B = 8192
ITERS = 50
# name -> (x widths, deps, relation_mlp hidden units per tower: [] = none)
SHAPES = {"taobao": ([64, 64], [[], [0]], [[], [64]]),
          "chain4": ([64, 64, 64, 64], [[], [0], [0, 1], [1, 2]], [[], [64, 32], [64, 32], [32, 16]])}


def chain_pass(dev, hx, deps, hidden):
    from torcheasyrec_amd.gate_ops import relation_chain, relation_chain_ok

    torch.manual_seed(0)
    xs = [torch.randn(B, w, device=dev).requires_grad_(True) for w in hx]
    widths, mlps = [], []
    for t, hu in enumerate(hidden):
        mlps.append(MLP(hx[t] + sum(widths[d] for d in deps[t]), hu).to(dev) if hu else None)
        widths.append(hu[-1] if hu else hx[t])
    gouts = [torch.randn(B, w, device=dev) / B for w in widths]
    layers = [[] if m is None else [(lin.weight, lin.bias) for lin in m.linears()] for m in mlps]
    params = [p for lay in layers for wb in lay for p in wb]
    assert relation_chain_ok(xs, deps, layers)

    def run():
        if rank_model.FUSED_RELATION_CHAIN:
            rs = relation_chain(xs, deps, layers)
        else:
            rs = []
            for t, m in enumerate(mlps):
                rs.append(xs[t] if m is None else m(torch.cat([xs[t]] + [rs[d] for d in deps[t]], dim=1)))
        torch.autograd.grad(rs, xs + params, gouts)

    return run


def timed(run, fused, n):
    rank_model.FUSED_RELATION_CHAIN = fused
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n  # us per pass


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    default = rank_model.FUSED_RELATION_CHAIN
    _lib.use_native()
    dev = torch.device("cuda", 0)
    work = {name: chain_pass(dev, *shape) for name, shape in SHAPES.items()}
    if mode == "trace":
        rank_model.FUSED_RELATION_CHAIN = sys.argv[2] == "fused"
        for run in work.values():
            for _ in range(ITERS):
                run()
        torch.cuda.synchronize()
        print(f"{sys.argv[2]}: {ITERS} forward + backward passes of each of {list(work)}")
        return
    out = {"B": B, "iters_per_round": ITERS, "shapes": {k: {"x": v[0], "deps": v[1], "relation_mlp": v[2]} for k, v in SHAPES.items()},
           "us_per_pass": {}}
    for name, run in work.items():
        for fused in (True, False):  # warm-up of both forms
            timed(run, fused, 10)
        rounds = {"fused": [], "literal": []}
        for _ in range(6):  # alternating: both forms see the same box
            rounds["fused"].append(timed(run, True, ITERS))
            rounds["literal"].append(timed(run, False, ITERS))
        out["us_per_pass"][name] = {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "max": max(v)} for k, v in rounds.items()}
        print(name, json.dumps(out["us_per_pass"][name]), flush=True)
    rank_model.FUSED_RELATION_CHAIN = default
    print(json.dumps(out))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
