"""`MaskNetModule` (torcheasyrec_amd/masknet.py) on tzr_ln_mask_fwd / tzr_ln_mask_bwd (csrc/ln_mask.hip) against the reference's
own module (tests/golden/reference_masknet_vectors.npz, LayerNorm weights and biases random) and the float64 restatement of the
literal module (tests/masknet_ref.py).

Bound, per tensor kind: |ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the distance of the reference's stored
result to float64 on the same inputs, the largest over the tensors of the kind -- never anything the code under test computed.
Kinds: y, gx, and one per parameter of the module with the blocks taken together (`g:mask_blocks.*.ffn.0.bias` is that
gradient of every block), as tests/test_cross_net.py takes the layers of the cross network together: the blocks are instances of
one computation, and the reference's own distance on `ffn.0.bias` at B = 6 is 4.6e-6, 3.8e-7 and 3.6e-7 for its three blocks.  The
stored cases hold no ReLU pre-activation within 2^-16 of zero (the generator asserts it; checked again here), so no row is
left out."""
import os
import re

import numpy as np
import pytest
import torch

import masknet_ref as ref
from torcheasyrec_amd import _lib
from torcheasyrec_amd import masknet
from torcheasyrec_amd.masknet import MaskBlock, MaskNetModule

VEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_masknet_vectors.npz"))
CASES = {"b6_d24_n3_h16_par": (6, 24, 3, 16, True, 2.0), "b6_d24_n3_h16_ser": (6, 24, 3, 16, False, 2.0),
         "b37_d429_n2_h65_par": (37, 429, 2, 65, True, 0.02)}


def _count_calls():
    """(forward, backward) calls of the row kernels' entry points since this call; restored by the `dev` fixture's next use_library"""
    lib, n = _lib.lib(), [0, 0]
    fwd, bwd = lib.tzr_ln_mask_fwd, lib.tzr_ln_mask_bwd

    def f(*a):
        n[0] += 1
        return fwd(*a)

    def b(*a):
        n[1] += 1
        return bwd(*a)

    lib.tzr_ln_mask_fwd, lib.tzr_ln_mask_bwd = f, b

    def done():
        lib.tzr_ln_mask_fwd, lib.tzr_ln_mask_bwd = fwd, bwd
        return tuple(n)

    return done


def _kind_of(key):
    """the tensor kind of a parameter's gradient: its state-dict key with the block's index left open"""
    return "g:" + re.sub(r"^mask_blocks\.\d+\.", "mask_blocks.*.", key)


def _load(tag):
    B, D, n, H, parallel, ratio = CASES[tag]
    keys = [str(k) for k in VEC[f"keys/{tag}"]]
    sd = {k: torch.from_numpy(VEC[f"{tag}/p:{k}"]) for k in keys}
    x, gy = torch.from_numpy(VEC[f"{tag}/x"]), torch.from_numpy(VEC[f"{tag}/gy"])
    members = {"y": ["y"], "gx": ["gx"]}
    for k in keys:
        members.setdefault(_kind_of(k), []).append(f"g:{k}")
    kinds = list(members)
    each = ref.masknet_literal(x, sd, n, parallel, gy)
    assert int(each["kink"].sum()) == 0
    want = {kind: [each[name][0] for name in names] for kind, names in members.items()}
    gaps = {k: float(VEC[f"ref_gap/{tag}/{k}"]) for k in kinds}
    stored = {kind: [torch.from_numpy(VEC[f"{tag}/{name}"]) for name in names] for kind, names in members.items()}
    for k in kinds:  # the stored results are the reference's: the restatement reproduces them to the stored gap
        assert abs(ref.rel_err(stored[k], want[k]) - gaps[k]) <= 1e-12, k
    return x, gy, sd, keys, members, want, gaps


def _module(dev, tag, sd):
    B, D, n, H, parallel, ratio = CASES[tag]
    m = MaskNetModule(D, n, {"hidden_dim": H, "reduction_ratio": ratio}, top_mlp=None, use_parallel=parallel)
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def _run(m, x, gy, members=None):
    """-> kind -> tensors; without `members` every tensor is a kind of its own"""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    y = m(x)
    y.backward(gy)
    each = {"y": y.detach(), "gx": x.grad}
    each.update({f"g:{k}": p.grad for k, p in m.named_parameters()})
    if members is None:
        return {k: [v] for k, v in each.items()}
    return {kind: [each[name] for name in names] for kind, names in members.items()}


@pytest.mark.parametrize("tag", list(CASES))
def test_module_matches_the_reference_module(dev, tag):
    B, D, n, H, parallel, ratio = CASES[tag]
    x, gy, sd, keys, members, want, gaps = _load(tag)
    kinds = list(members)
    assert len(kinds) == 12  # y, gx, ln_emb's two and a block's eight
    m = _module(dev, tag, sd)
    assert list(m.state_dict()) == keys
    assert all(float((sd[k] - (1.0 if k.endswith("weight") else 0.0)).abs().max()) > 0 for k in keys if "ln_emb" in k or "ffn.1" in k)
    calls = _count_calls()
    got = _run(m, x.to(dev), gy.to(dev), members)
    assert calls() == ((2, 2) if parallel else (n + 1, n + 1))
    assert got["y"][0].shape == (B, n * H if parallel else H)
    ref.check(got, want, gaps, f"{tag} on {dev.type}", kinds)
    again = _run(m, x.to(dev), gy.to(dev), members)
    assert all(torch.equal(a, b) for k in kinds for a, b in zip(got[k], again[k])), "two runs of the same case differ"


@pytest.mark.parametrize("tag", list(CASES))
def test_switch_off_runs_the_literal_loop(dev, monkeypatch, tag):
    monkeypatch.setattr(masknet, "FUSED_MASKNET", False)
    x, gy, sd, keys, members, want, gaps = _load(tag)
    m = _module(dev, tag, sd)
    calls = _count_calls()
    got = _run(m, x.to(dev), gy.to(dev), members)
    assert calls() == (0, 0)
    ref.check(got, want, gaps, f"literal {tag} on {dev.type}", list(members))


@pytest.mark.parametrize("how", ["wide", "many", "double"])
def test_literal_loop_outside_the_kernels_limits(dev, how):
    D, n, H, dtype = {"wide": (1025, 2, 8, torch.float32), "many": (12, 9, 8, torch.float32), "double": (12, 2, 8, torch.float64)}[how]
    torch.manual_seed(5)
    m = MaskNetModule(D, n, {"hidden_dim": H, "reduction_ratio": 0.5}, use_parallel=True).to(dev).to(dtype)
    calls = _count_calls()
    x = torch.randn(4, D, dtype=dtype, device=dev, requires_grad=True)
    y = m(x)
    y.sum().backward()
    assert calls() == (0, 0) and y.shape == (4, n * H) and bool(torch.isfinite(x.grad).all())


def test_one_block_and_a_top_mlp(dev, monkeypatch):
    """n = 1 in both modes (the Function returns one tensor, not a tuple) with a top MLP behind; gap = the literal fp32 form's
    distance to a float64 run of the literal form, both on the CPU"""
    for parallel in (True, False):
        def twin(dtype):
            t = MaskNetModule(20, 1, {"hidden_dim": 12}, top_mlp={"hidden_units": [6]}, use_parallel=parallel).to(dtype)
            t.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in m.state_dict().items()})
            return t

        torch.manual_seed(11)
        m = MaskNetModule(20, 1, {"hidden_dim": 12}, top_mlp={"hidden_units": [6]}, use_parallel=parallel).to(dev)
        x, gy = torch.randn(9, 20), torch.randn(9, 6)
        calls = _count_calls()
        got = _run(m, x.to(dev), gy.to(dev))
        assert calls() == (2, 2) and m.output_dim() == 6
        monkeypatch.setattr(masknet, "FUSED_MASKNET", False)
        want = _run(twin(torch.float64), x.double(), gy.double())
        lit = _run(twin(torch.float32), x, gy)
        monkeypatch.setattr(masknet, "FUSED_MASKNET", True)
        kinds = list(got)
        ref.check(got, want, {k: ref.rel_err(lit[k], want[k]) for k in kinds}, f"one block, parallel={parallel} on {dev.type}", kinds)


def test_state_dict_keys_are_the_references():
    m = MaskNetModule(24, 2, {"hidden_dim": 16}, top_mlp={"hidden_units": [8, 4]}, use_parallel=True)
    theirs = [str(k) for k in VEC["keys/with_top_mlp"]]
    # the top MLP is the package's `MLP`, whose Linear of layer i is `mlp.<2i>` where the reference's is `mlp.<i>.perceptron.0`
    # (so for every model built here); everything else is key for key the reference's
    mine = list(m.state_dict())
    assert [k for k in mine if not k.startswith("top_mlp.")] == [k for k in theirs if not k.startswith("top_mlp.")]
    assert [k for k in mine if k.startswith("top_mlp.")] == ["top_mlp.mlp.0.weight", "top_mlp.mlp.0.bias", "top_mlp.mlp.2.weight", "top_mlp.mlp.2.bias"]
    assert [k for k in theirs if k.startswith("top_mlp.")] == [f"top_mlp.mlp.{i}.perceptron.0.{w}" for i in (0, 1) for w in ("weight", "bias")]
    assert m.output_dim() == 4 and MaskNetModule(24, 2, {"hidden_dim": 16}).output_dim() == 32
    assert MaskNetModule(24, 3, {"hidden_dim": 16}, use_parallel=False).output_dim() == 16


def test_aggregation_dim_follows_the_references_constructor():
    # reduction_ratio non-zero (the proto default 1.0 always arrives): int(input_dim * ratio), whatever aggregation_dim says
    assert MaskBlock(24, 24, 16).aggregation_dim == 24
    assert MaskBlock(24, 24, 16, reduction_ratio=2.0).aggregation_dim == 48
    assert MaskBlock(24, 24, 16, reduction_ratio=0.3).aggregation_dim == 7
    assert MaskBlock(24, 24, 16, reduction_ratio=1.0, aggregation_dim=5).aggregation_dim == 24
    # the configured aggregation_dim counts only with reduction_ratio 0; both zero is refused
    assert MaskBlock(24, 24, 16, reduction_ratio=0, aggregation_dim=5).aggregation_dim == 5
    with pytest.raises(ValueError, match="aggregation_dim or reduction_ratio"):
        MaskBlock(24, 24, 16, reduction_ratio=0, aggregation_dim=0)
    # input_dim is the block's FEATURE input: in serial mode the hidden width for blocks i >= 1 (the mask input stays the embedding)
    m = MaskNetModule(24, 3, {"hidden_dim": 16, "reduction_ratio": 2.0}, use_parallel=False)
    assert [b.aggregation_dim for b in m.mask_blocks] == [48, 32, 32]
    assert [tuple(b.mask_generator[0].weight.shape) for b in m.mask_blocks] == [(48, 24), (32, 24), (32, 24)]
    assert [tuple(b.mask_generator[2].weight.shape) for b in m.mask_blocks] == [(24, 48), (16, 32), (16, 32)]
    assert [tuple(b.ffn[0].weight.shape) for b in m.mask_blocks] == [(16, 24), (16, 16), (16, 16)]
    p = MaskNetModule(24, 3, {"hidden_dim": 16, "reduction_ratio": 2.0}, use_parallel=True)
    assert [b.aggregation_dim for b in p.mask_blocks] == [48, 48, 48]
