"""Generate tests/golden/reference_masknet_vectors.npz by RUNNING the reference's own `MaskNetModule`.

Run in the authoring container only (needs the reference checkout; the GPU box has none):

    python tests/golden/make_reference_masknet_vectors.py

`tzrec/modules/masknet.py:20-161` is imported from where it lies through the import shim of make_reference_module_vectors.py
and executed on CPU in fp32, without a top MLP (that part is `MLP`, covered by reference_module_vectors.npz).  The reference
initialises every LayerNorm to weight 1 and bias 0, which would hide gamma and beta: they are set to random values first.

Per case (B, D, n, H, parallel, reduction_ratio): the input `x`, every parameter `p:<state-dict key>`, the output gradient
`gy`, and the reference's `y`, `gx`, `g:<state-dict key>`.  `ref_gap/<case>/<kind>` is the reference's own distance to a float64
evaluation of the same module on the same values, max |fp32 - fp64| / max(1, |fp64|) over the tensors of the kind: the yardstick
the tests scale their bound with.  Kinds: y, gx, and one per parameter of the module with the blocks taken together, as
make_reference_cross_vectors.py takes the layers together (`g:ln_emb.weight`, `g:mask_blocks.*.ffn.0.bias`, ...): the blocks
are instances of one computation, and at B = 6 a single instance's distance is one draw of a wide spread.  `keys/<case>` is the reference's list of state-dict keys, `keys/with_top_mlp` that of a
module with `top_mlp { hidden_units: [8, 4] }`.

No case may hold a ReLU pre-activation within 2^-16 of zero in float64 (the fp32 run could take the other side there): the
script asserts it and moves on to the next seed otherwise.
"""
import copy
import importlib
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_module_vectors import _np, install_reference_imports  # noqa: E402

CASES = {"b6_d24_n3_h16_par": (6, 24, 3, 16, True, 2.0), "b6_d24_n3_h16_ser": (6, 24, 3, 16, False, 2.0),
         "b37_d429_n2_h65_par": (37, 429, 2, 65, True, 0.02)}  # (ratio 0.02: an aggregation layer 8 wide keeps the file well under 1 MiB)
KINK = 2.0 ** -16


def kind_of(key):
    """the tensor kind of a parameter's gradient: its state-dict key with the block's index left open"""
    return "g:" + re.sub(r"^mask_blocks\.\d+\.", "mask_blocks.*.", key)


def _run(mod, x, gy):
    """forward + backward; the pre-activations of every ReLU are collected by hooks on the nn.ReLU modules"""
    pre = []
    hooks = [m.register_forward_hook(lambda _m, inp, _out: pre.append(inp[0].detach())) for m in mod.modules()
             if isinstance(m, torch.nn.ReLU)]
    mod.zero_grad()
    x = x.clone().requires_grad_(True)
    y = mod(x)
    y.backward(gy)
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), "gx": x.grad}
    out.update({f"g:{k}": p.grad for k, p in mod.named_parameters()})
    return out, pre


def _case(mn_mod, B, D, n, H, parallel, ratio, seed):
    torch.manual_seed(seed)
    mod = mn_mod.MaskNetModule(D, n, {"hidden_dim": H, "reduction_ratio": ratio}, top_mlp=None, use_parallel=parallel)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape))
    x = torch.randn(B, D)
    gy = torch.randn(B, mod.output_dim())
    r32, _ = _run(mod, x, gy)
    r64, pre = _run(copy.deepcopy(mod).double(), x.double(), gy.double())
    if any(bool((p.abs() < KINK).any()) for p in pre):
        return None
    return mod, x, gy, r32, r64


def main():
    install_reference_imports()
    mn_mod = importlib.import_module("tzrec.modules.masknet")
    torch.set_num_threads(1)
    out = {}
    for tag, (B, D, n, H, parallel, ratio) in CASES.items():
        seed = 20261019
        while (res := _case(mn_mod, B, D, n, H, parallel, ratio, seed)) is None:
            seed += 1
        mod, x, gy, r32, r64 = res
        assert not any(bool((p.abs() < KINK).any()) for p in _run(copy.deepcopy(mod).double(), x.double(), gy.double())[1])
        out[f"{tag}/x"], out[f"{tag}/gy"] = _np(x), _np(gy)
        out[f"keys/{tag}"] = np.array(list(mod.state_dict()))
        for k, p in mod.state_dict().items():
            out[f"{tag}/p:{k}"] = _np(p)
        for name in r32:
            out[f"{tag}/{name}"] = _np(r32[name])
            a, e = r32[name].double(), r64[name]
            gap = float(((a - e).abs() / e.abs().clamp(min=1.0)).max())
            kind = f"ref_gap/{tag}/{kind_of(name[2:]) if name.startswith('g:') else name}"
            out[kind] = np.float64(max(gap, float(out.get(kind, 0.0))))
        print(tag, "seed", seed, {k: f"{float(out[f'ref_gap/{tag}/{k}']):.2e}" for k in ("y", "gx", "g:ln_emb.weight")})
    top = mn_mod.MaskNetModule(24, 2, {"hidden_dim": 16}, top_mlp={"hidden_units": [8, 4]}, use_parallel=True)
    out["keys/with_top_mlp"] = np.array(list(top.state_dict()))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_masknet_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
