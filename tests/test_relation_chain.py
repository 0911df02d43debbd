"""gate_ops.relation_chain (tzr_relation_chain_fwd / _bwd, csrc/relation_chain.hip): every Bayesian relation tower of a DBMTL
model in one launch forward and two backward, against the literal cat / Linear / ReLU form evaluated in float64 on the CPU
(tests/relation_chain_ref.py).  Per kind (h, dx, dW, db): max |got - fp64| / max(1, |fp64|) at or below 4 x the distance of
torch's own fp32 literal form to the float64 result on the same inputs, floor 2^-20.  The inputs are settled: no float64
pre-activation lies within 2^-12 of zero, so no ReLU mask can differ; no element is left out of any comparison."""
import pytest
import torch

import relation_chain_ref as ref
from torcheasyrec_amd import _lib


def to_dev(xs, layers, gouts, dev, strided=False):
    """leaves on `dev`; a shared x stays one object; strided: every x is the column slice [:, 4 : 4 + Hx] of a buffer 12 wider"""
    def put(x):
        if strided:
            buf = torch.zeros(x.shape[0], x.shape[1] + 12)
            buf[:, 4:4 + x.shape[1]] = x
            return buf.to(dev)[:, 4:4 + x.shape[1]].requires_grad_(True)
        return x.to(dev).clone().requires_grad_(True)

    moved = {id(x): put(x) for x in ref.unique(xs)}
    return ([moved[id(x)] for x in xs], [[(w.to(dev).clone().requires_grad_(True), b.to(dev).clone().requires_grad_(True)) for w, b in lay] for lay in layers],
            [None if g is None else g.to(dev) for g in gouts])


def run(xs, deps, layers, gouts):
    from torcheasyrec_amd.gate_ops import relation_chain, relation_chain_ok

    assert relation_chain_ok(xs, deps, layers)
    rs, hs = relation_chain(xs, deps, layers, hidden=True)
    for t, lay in enumerate(layers):
        assert (rs[t] is xs[t]) == (not lay)  # (a tower without layers: its input itself, nothing copied)
    pairs = [(r, g) for r, g in zip(rs, gouts) if g is not None]
    ux = ref.unique(xs)
    ins = ux + [p for lay in layers for wb in lay for p in wb]
    grads = torch.autograd.grad([r for r, _ in pairs], ins, [g for _, g in pairs], allow_unused=True)
    assert all(g is not None for g in grads)  # (one Function: every input gets a gradient, zeros where nothing flows)
    n = len(ux)
    return {"h": [h.detach() for ht in hs for h in ht], "dx": list(grads[:n]), "dW": list(grads[n::2]), "db": list(grads[n + 1::2])}


def check_case(dev, B, hx, deps, widths, seed, null=(), shared=None, strided=False):
    xs, layers, gouts = ref.draw(B, hx, deps, widths, seed, shared)
    gouts = [None if t in null else g for t, g in enumerate(gouts)]
    want = ref.literal(xs, deps, layers, gouts, torch.float64)
    gaps = ref.gaps(xs, deps, layers, gouts, want)
    dxs, dlayers, dgouts = to_dev(xs, layers, gouts, dev, strided)
    got = run(dxs, deps, dlayers, dgouts)
    what = f"B{B} hx{hx} deps{deps} widths{widths} null{tuple(null)} shared{shared} strided={strided} on {dev.type}"
    ref.check(got, want, gaps, what, ref.KINDS)
    again = run(dxs, deps, dlayers, dgouts)
    for kind in ref.KINDS:
        assert all(torch.equal(a, b) for a, b in zip(got[kind], again[kind])), f"{what} {kind}: two runs differ"
    return got, want


CHAIN = ([[], [0], [1]], "chain a -> b -> c")


@pytest.mark.parametrize("B", [1, 3, 15, 16, 17, 33])
def test_chain_at_every_row_tail(dev, B):
    """a -> b -> c with 1, 2 and 1 layers: less than a row block, exactly one, one row more, two and a row"""
    check_case(dev, B, [20, 20, 4], CHAIN[0], [[12], [36, 12], [4]], seed=B)


def test_a_workgroup_runs_its_row_loop_twice(dev):
    """The row passes launch min(ceil(B / 16), 512) workgroups, and workgroup i takes the row blocks i, i + grid, ..: with
    B = 512 * 16 + 17 = 8209 there are 514 blocks, so workgroups 0 and 1 take two blocks each, the second of workgroup 1 a
    partial one (one row).  The weight-gradient workgroups sum all 8209 rows.  Widths of 4: seconds on the emulator."""
    check_case(dev, 512 * 16 + 17, [4, 4], [[], [0]], [[4], [4]], seed=7)


# (Hx, layer widths): less than one column tile (4, 12), a ragged last tile (36, 68), more tiles than waves and the limit (128);
# 1, 2 and 4 layers; Hx = 260 makes the first layer's K run over more than one staged chunk of 256 columns
@pytest.mark.parametrize("hx,widths", [(4, [128]), (20, [68, 36]), (64, [36, 4, 12, 68]), (260, [12]), (260, [128, 128]), (64, [4]),
                                       (4, [12, 128, 68, 4])])
def test_widths_and_depths(dev, hx, widths):
    """a two-tower chain whose second tower has the widths under test; the first one's 68 units make its segment ragged"""
    check_case(dev, 19, [hx, hx], [[], [0]], [[68], widths], seed=hx + sum(widths))


GRAPHS = {
    "chain": ([20, 12, 8], [[], [0], [1]], [[12], [12, 8], [16]]),
    "fan_in": ([20, 12, 8], [[], [], [0, 1]], [[12], [36], [16, 8]]),
    "fan_out": ([20, 12, 8], [[], [0], [0]], [[12], [36], [16]]),
    "no_deps": ([20, 12], [[], []], [[12, 4], [8]]),
    # tower 0 has no layers and is read by 1 and 2 (its dx: stored by 2, added to by 1); tower 3 has none and nobody reads it
    "l0_consumed": ([20, 12, 8, 4], [[], [0], [1, 0], [2]], [[], [12], [16, 8], []]),
    # the first layer's K spans two chunks, with an L = 0 segment and a computed one behind x
    "l0_wide": ([260, 64, 8], [[], [], [0, 1]], [[], [68], [36]]),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graphs(dev, name):
    hx, deps, widths = GRAPHS[name]
    check_case(dev, 21, hx, deps, widths, seed=len(name))


def test_two_towers_share_one_input(dev):
    """towers 0 and 1 read the same tensor (towers without their own mlp): its gradient is the sum of both; also with tower 0
    without layers"""
    check_case(dev, 18, [20, 20, 8], [[], [0], [0, 1]], [[12], [12], [8]], seed=3, shared={1: 0})
    check_case(dev, 18, [20, 20], [[], [0]], [[], [12]], seed=4, shared={1: 0})


def test_a_tower_without_an_outside_gradient(dev):
    """tower 0's r gets a gradient from its consumer only; tower 2's from nowhere: its parameters' gradients are exact zeros"""
    got, _ = check_case(dev, 18, [20, 12, 8], [[], [0], []], [[12], [8], [4]], seed=5, null=(0, 2))
    assert float(got["dW"][2].abs().max()) == 0.0 and float(got["db"][2].abs().max()) == 0.0 and float(got["dx"][2].abs().max()) == 0.0
    assert float(got["dW"][0].abs().max()) > 0.0


def test_inputs_as_column_slices_of_wider_buffers(dev):
    check_case(dev, 18, [20, 12, 8], [[], [0], [1, 0]], [[12], [], [8, 4]], seed=6, strided=True)


def test_forward_under_no_grad(dev):
    from torcheasyrec_amd.gate_ops import relation_chain

    hx, deps, widths = GRAPHS["l0_consumed"]
    xs, layers, gouts = ref.draw(9, hx, deps, widths, seed=8)
    want = ref.literal(xs, deps, layers, gouts, torch.float64)
    gaps = ref.gaps(xs, deps, layers, gouts, want)
    dxs, dlayers, _ = to_dev(xs, layers, gouts, dev)
    with torch.no_grad():
        rs, hs = relation_chain(dxs, deps, dlayers, hidden=True)
    assert not any(r.requires_grad for r in rs if r is not dxs[0] and r is not dxs[3])
    ref.check({"h": [h for ht in hs for h in ht]}, want, gaps, f"no_grad on {dev.type}", ("h",))


def test_relation_chain_ok_refuses_what_the_kernel_does_not_take(dev):
    from torcheasyrec_amd.gate_ops import relation_chain_ok

    def case(B=6, hx=(8, 8), widths=((8,), (8,)), deps=((), (0,)), dtype=torch.float32):
        new = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        xs, layers, rw = [new(B, h) for h in hx], [], []
        for t, ws in enumerate(widths):
            K, lay = hx[t] + sum(rw[d] for d in deps[t] if d < t), []
            for N in ws:
                lay.append((new(N, K), new(N)))
                K = N
            layers.append(lay)
            rw.append(K if ws else hx[t])
        return xs, [list(d) for d in deps], layers

    assert relation_chain_ok(*case()) and relation_chain_ok(*case(hx=(1024, 8), widths=((128, 128, 128, 128), ())))
    assert not relation_chain_ok(*case(hx=(6, 8))) and not relation_chain_ok(*case(hx=(1028, 8)))
    assert not relation_chain_ok(*case(widths=((6,), (8,)))) and not relation_chain_ok(*case(widths=((132,), (8,))))
    assert not relation_chain_ok(*case(widths=((8, 8, 8, 8, 8), (8,)))) and not relation_chain_ok(*case(B=0))
    assert not relation_chain_ok(*case(dtype=torch.float16))
    assert not relation_chain_ok(*case(deps=((), (1,)))) and not relation_chain_ok(*case(deps=((1,), ())))
    assert not relation_chain_ok(*case(hx=(8,) * 3, widths=((8,),) * 3, deps=((), (), (0, 0))))
    assert not relation_chain_ok(*case(hx=(8,) * 9, widths=((8,),) * 9, deps=((),) * 9))
    xs, deps, layers = case()
    odd = torch.zeros(6, 11, dtype=torch.float32, device=dev)[:, :8]  # an odd row stride
    wide = torch.zeros(6, 20, dtype=torch.float32, device=dev)
    assert not relation_chain_ok([xs[0], odd], deps, layers) and not relation_chain_ok([xs[0], wide[:, 2:10]], deps, layers)
    assert relation_chain_ok([xs[0], wide[:, 4:12]], deps, layers)
    assert (_lib.RELATION_CHAIN_MAX_TOWERS, _lib.RELATION_CHAIN_MAX_LAYERS, _lib.RELATION_CHAIN_MAX_WIDTH, _lib.RELATION_CHAIN_MAX_X) == (8, 4, 128, 1024)
