"""hstu.STULayer / STUStack: the reference's parameter names, and a two-layer stack against the same layers restated in float64 on
tests/hstu_ref.py -- the output and every parameter and input gradient under the project's rule (max |got - fp64| / max(1, |fp64|)
at or below 4 x the float32 restatement's own distance, floor 2^-20), dropout 0, each layer taking the fused kernels exactly once."""
import pytest
import torch
import torch.nn.functional as F

import hstu_ref as ref

NAMES = ("_input_norm_weight", "_input_norm_bias", "_uvqk_weight", "_uvqk_beta", "_output_weight", "_output_norm_weight", "_output_norm_bias")
SHAPES = {
    "targets_and_contextual": dict(lengths=[0, 5, 17, 66], E=12, H=2, Dv=8, Da=4, max_seq_len=70, num_targets=[0, 2, 17, 3], c=3, L=0, group_norm=False),
    "group_norm": dict(lengths=[3, 33, 1], E=8, H=3, Dv=4, Da=8, max_seq_len=40, num_targets=None, c=0, L=6, group_norm=True),
}


def layer_ref(x, w, p, c, dtype):
    """one STU layer on float tensors `w` (NAMES order) with the attention of hstu_ref"""
    inw, inb, uw, ub, ow, onw, onb = w
    H, Dv, Da, N = c["H"], c["Dv"], c["Da"], x.shape[0]
    uvqk = torch.addmm(ub, F.layer_norm(x, (c["E"],), inw, inb, 1e-6), uw)
    u, v, q, k = torch.split(uvqk, [Dv * H, Dv * H, Da * H, Da * H], dim=1)
    u = F.silu(u)
    attn = ref.attention({**p, "alpha": Da ** -0.5}, q.reshape(N, H, Da), k.reshape(N, H, Da), v.reshape(N, H, Dv), dtype).reshape(N, H * Dv)
    if c["group_norm"]:
        y = u * F.group_norm(attn.view(N, H, Dv), H, onw, onb, 1e-6).view(N, H * Dv)
    else:
        y = u * F.layer_norm(attn, (H * Dv,), onw, onb, 1e-6)
    return torch.addmm(x, torch.cat([u, attn, y], dim=1), ow)


def stack_ref(x, weights, g, p, c, dtype):
    x = x.detach().to(dtype).clone().requires_grad_(True)
    ws = [[t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in w] for w in weights]
    y = x
    for w in ws:
        y = layer_ref(y, w, p, c, dtype)
    leaves = [x] + [t for w in ws for t in w]
    return {"out": [y.detach()], "grads": list(torch.autograd.grad((y * g.to(dtype)).sum(), leaves))}


def test_the_state_dict_keys_are_the_references():
    from torcheasyrec_amd.hstu import STULayer

    assert set(STULayer(8, 2, 4, 4).state_dict()) == set(NAMES)
    for kwargs, word in ((dict(sla_k1=2), "sla_k1"), (dict(causal=False), "causal")):
        with pytest.raises(NotImplementedError, match=word):
            STULayer(8, 2, 4, 4, **kwargs)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_a_two_layer_stack_against_float64(dev, name):
    from torcheasyrec_amd import hstu

    c = SHAPES[name]
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(name))
    offsets = torch.tensor([0] + c["lengths"], dtype=torch.int64).cumsum(0)
    N = int(offsets[-1])
    nt = None if c["num_targets"] is None else torch.tensor(c["num_targets"], dtype=torch.int64)
    x, g = torch.randn(N, c["E"], generator=gen), torch.randn(N, c["E"], generator=gen)
    layers = [hstu.STULayer(c["E"], c["H"], c["Dv"], c["Da"], output_dropout_ratio=0.0, max_attn_len=c["L"], contextual_seq_len=c["c"],
                            use_group_norm=c["group_norm"], recompute_y=False, sort_by_length=False) for _ in range(2)]
    for layer in layers:  # every parameter off its constant start
        for t in layer.parameters():
            t.data.add_(0.1 * torch.randn(t.shape, generator=gen))
    with pytest.raises(NotImplementedError, match="truncate"):
        hstu.STUStack(layers, truncate_split_layer=1, truncate_tail_len=4)
    stack = hstu.STUStack(layers).to(dev)
    weights = [[getattr(layer, n) for n in NAMES] for layer in layers]
    p = {"offsets": offsets, "max_seq_len": c["max_seq_len"], "L": c["L"], "c": c["c"], "scaling_seqlen": -1, "num_targets": nt}
    want, r32 = stack_ref(x, weights, g, p, c, torch.float64), stack_ref(x, weights, g, p, c, torch.float32)
    xd = x.to(dev).requires_grad_(True)
    before = hstu._HstuMhaFn.calls
    out = stack(xd, offsets.to(dev), c["max_seq_len"], None if nt is None else nt.to(dev))
    assert hstu._HstuMhaFn.calls == before + 2  # each layer took the kernels exactly once
    grads = torch.autograd.grad((out * g.to(dev)).sum(), [xd] + [t for w in weights for t in w])
    got = {"out": [out.detach()], "grads": list(grads)}
    ref.check(got, want, {k: ref.rel_err(r32[k], want[k]) for k in want}, f"{name} on {dev.type}", ("out", "grads"))
