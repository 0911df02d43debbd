"""rocket.distill_losses (tzr_distill_loss_fwd / _bwd, csrc/distill_loss.hip): every similarity term of a Rocket Launching step and
the hint loss in one launch, against the reference's literal form evaluated in float64 on the CPU (tests/distill_loss_ref.py).
Per kind (each sim_p, hint, each d light_p, d logits_light): max |got - fp64| / max(1, |fp64|) at or below 4 x the distance of
torch's own fp32 literal form to the float64 result on the same inputs, floor 2^-20; no element is left out.  The upstream
gradients are distinct per term and none of them 1 (distill_loss_ref.upstream).

The layout is amm_loss.hip's: one wave a sample, four samples a workgroup, no loop over the batch -- B = 1, 3 (a partial
workgroup), 4 (a full one), 5 and 67 (more than one) are the block shapes there are; the finishing sum's sixteen chains take
eight rows a pass, so B = 517 (130 workgroups) runs their loop twice.  What differs: a wave walks its row in steps of 256 floats,
so besides one float4, two lanes, a lane short of sixteen / of the wave and full ones (4, 8, 60, 64, 252, 256), W = 260 takes a
second step with one lane and 1020 / 1024 a fourth with 63 / 64; and a wave loops over the pairs, P in {0, 1, 2, 8}."""
import pytest
import torch

import distill_loss_ref as ref
from torcheasyrec_amd import _lib

MODES = {"cosine": True, "distance": False}


def put(x, dev, strided=False, grad=True):
    """a leaf on `dev`; strided: the column slice [:, 4 : 4 + W] of a buffer 12 wider"""
    if strided:
        buf = torch.zeros(x.shape[0], x.shape[1] + 12)
        buf[:, 4:4 + x.shape[1]] = x
        return buf.to(dev)[:, 4:4 + x.shape[1]].requires_grad_(grad)
    return x.to(dev).clone().requires_grad_(grad)


def counted(fn):
    """-> (fn's result, the number of tzr_distill_loss_fwd calls it made)"""
    calls, L = [], _lib.lib()
    orig = L.tzr_distill_loss_fwd
    L.tzr_distill_loss_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        return fn(), len(calls)
    finally:
        L.tzr_distill_loss_fwd = orig


def run(dev, ls, bs, ll, lb, w, cosine, g=None, strided=False, fused=True):
    from torcheasyrec_amd import rocket

    P = len(ls)
    g = ref.upstream(P) if g is None else g
    dls, dbs = [put(t, dev, strided) for t in ls], [put(t, dev, strided) for t in bs]
    dll, dlb = put(ll, dev), put(lb, dev)
    dw = None if w is None else w.to(dev)
    if fused:
        assert rocket.FUSED_DISTILL_LOSS and rocket.distill_losses_ok(dls, dbs, dll, dlb, dw)
    (sims, hint), n = counted(lambda: rocket.distill_losses(dls, dbs, dll, dlb, cosine, dw))
    assert n == (1 if fused else 0) and len(sims) == P  # (the kernel, exactly once -- or the literal form and no kernel)
    total = sum(t * c for t, c in zip(tuple(sims) + (hint,), g) if c is not None)
    grads = torch.autograd.grad(total, dls + [dll] + dbs + [dlb], allow_unused=True)
    assert all(d is None for d in grads[P + 1:])  # (every booster operand is a constant)
    grads = [torch.zeros_like(t) if d is None else d for d, t in zip(grads[:P + 1], dls + [dll])]
    out = {f"sim{p}": [sims[p].detach()] for p in range(P)}
    out["hint"] = [hint.detach()]
    out.update({f"dl{p}": [grads[p]] for p in range(P)})
    out["dll"] = [grads[P]]
    return out


def check_case(dev, B, widths, C, cosine, weights=None, strided=False, seed=0):
    ls, bs, ll, lb, w = ref.draw(B, widths, C, seed, weights)
    want = ref.literal(ls, bs, ll, lb, cosine, w)
    gaps = ref.gaps(ls, bs, ll, lb, cosine, w, None, want)
    got = run(dev, ls, bs, ll, lb, w, cosine, strided=strided)
    ref.check(got, want, gaps, f"B{B} W{widths} C{C} cosine={cosine} weights={weights} strided={strided} on {dev.type}", ref.kinds(len(widths)))
    return got


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("B", [1, 3, 4, 5, 67])
def test_every_batch(dev, B, mode, weights):
    check_case(dev, B, (8, 12), 1, MODES[mode], weights, seed=B)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("W", [4, 8, 60, 64, 252, 256, 260, 1020, 1024])
def test_every_width_contiguous_and_as_a_column_slice(dev, W, mode, weights, strided):
    check_case(dev, 5, (W,), 1, MODES[mode], weights, strided=strided, seed=100 + W)


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_finishing_sums_chains_run_twice(dev, mode, weights):
    check_case(dev, 517, (8, 4), 1, MODES[mode], weights, seed=7)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("P", [0, 1, 2, 8])
def test_every_pair_count(dev, P, mode):
    """P = 0 is the hint loss alone (feature_based_distillation off); 8 is the limit"""
    check_case(dev, 5, tuple(4 * (1 + p % 3) for p in range(P)), 1, MODES[mode], "rand", seed=200 + P)


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_pairs_of_different_widths_in_one_call(dev, mode, weights):
    check_case(dev, 67, (64, 32, 8), 1, MODES[mode], weights, seed=11)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("C", [1, 2, 3])
def test_every_logit_width(dev, C, mode):
    """C = 1 here is [B, 1]-shaped logits as well as the squeezed [B] of the other tests"""
    check_case(dev, 5, (8,), C, MODES[mode], seed=300 + C)
    ls, bs, ll, lb, _ = ref.draw(67, (8,), 1, 310 + C)
    ll, lb = ll.reshape(-1, 1).repeat(1, C), lb.reshape(-1, 1) * torch.arange(1, C + 1)
    want = ref.literal(ls, bs, ll, lb, MODES[mode])
    ref.check(run(dev, ls, bs, ll, lb, None, MODES[mode]), want, ref.gaps(ls, bs, ll, lb, MODES[mode], None, None, want),
              f"[67, {C}] logits {mode} on {dev.type}", ref.kinds(1))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_all_weights_zero(dev, mode):
    """div_no_nan: every loss exactly 0, every gradient exactly 0, nothing non-finite"""
    ls, bs, ll, lb, w = ref.draw(5, (8, 64), 1, 30, "zero")
    got = run(dev, ls, bs, ll, lb, w, MODES[mode])
    for k in ref.kinds(2):
        assert bool(torch.isfinite(got[k][0]).all()) and float(got[k][0].abs().max()) == 0.0, k


@pytest.mark.parametrize("weights", [None, "rand"])
def test_all_zero_rows_take_the_clamp_branch(dev, weights):
    """F.normalize divides by max(|x|, 1e-12).  A zero light row has y = 0 and the gradient dy / 1e-12, of the order 1e9 -- checked
    on that row alone, so that it does not set the norm for the other rows, and the other rows without it.  A zero booster row is
    a zero target: that sample's cosine and gradient row are 0."""
    ls, bs, ll, lb, w = ref.draw(5, (8,), 1, 40, weights)
    ls[0][2] = 0.0
    bs[0][3] = 0.0
    want = ref.literal(ls, bs, ll, lb, True, w)
    r32 = ref.literal(ls, bs, ll, lb, True, w, dtype=torch.float32)
    got = run(dev, ls, bs, ll, lb, w, True)
    assert float(want["dl0"][0][2].abs().max()) > 1e8 and float(want["dl0"][0][3].abs().max()) == 0.0
    assert float(got["dl0"][0][3].abs().max()) == 0.0
    for name in ("the zero row", "the other rows"):
        def part(res):
            out = {k: [res[k][0].cpu()] for k in ("sim0", "hint", "dll")}
            t = res["dl0"][0].cpu()
            out["dl0"] = [t[2:3] if name == "the zero row" else torch.cat([t[:2], t[3:]])]
            return out

        w64 = part(want)
        ref.check(part(got), w64, {k: ref.rel_err(part(r32)[k], w64[k]) for k in w64}, f"{name} weights={weights} on {dev.type}", ref.kinds(1))


@pytest.mark.parametrize("weights", [None, "rand"])
def test_distance_of_equal_rows_gives_zero_gradient_rows(dev, weights):
    """light == booster under the distance function: sqrt'(0) is inf and the literal gradient 0 * inf = NaN; the kernel writes
    zero rows (documented in the kernel's header and DESIGN.md).  The other pair of the same call and the hint are as ever."""
    ls, bs, ll, lb, w = ref.draw(5, (8, 12), 1, 45, weights)
    bs[0] = ls[0].clone()
    got = run(dev, ls, bs, ll, lb, w, False)
    assert float(got["sim0"][0]) == 0.0 and torch.equal(got["dl0"][0].cpu(), torch.zeros(5, 8))
    want = ref.literal(ls, bs, ll, lb, False, w)
    assert not bool(torch.isfinite(want["dl0"][0]).any())  # (the literal form: NaN)
    rest = ("sim1", "hint", "dl1", "dll")
    gaps = ref.gaps(ls, bs, ll, lb, False, w, None, want)
    ref.check(got, want, gaps, f"the other terms weights={weights} on {dev.type}", rest)


def test_two_runs_are_bit_equal(dev):
    ls, bs, ll, lb, w = ref.draw(67, (64, 32, 260), 1, 50, "rand")
    for cosine in (True, False):
        a, b = run(dev, ls, bs, ll, lb, w, cosine), run(dev, ls, bs, ll, lb, w, cosine)
        for k in ref.kinds(3):
            assert torch.equal(a[k][0], b[k][0]), k


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("missing", [0, 1, 2])
def test_a_term_nobody_differentiates(dev, mode, missing):
    """upstream gradient None for sim_0, sim_1 or the hint: that operand's gradient is None or zeros, the others' as with all three"""
    ls, bs, ll, lb, w = ref.draw(5, (8, 12), 1, 60, "rand")
    g = ref.upstream(2)
    g[missing] = None
    want = ref.literal(ls, bs, ll, lb, MODES[mode], w, g)
    got = run(dev, ls, bs, ll, lb, w, MODES[mode], g)
    ref.check(got, want, ref.gaps(ls, bs, ll, lb, MODES[mode], w, g, want), f"no gradient for term {missing} {mode} on {dev.type}", ref.kinds(2))
    assert float(got[("dl0", "dl1", "dll")[missing]][0].abs().max()) == 0.0


def test_a_double_backward_goes_through_the_literal_form(dev):
    from torcheasyrec_amd import rocket

    for cosine in (True, False):
        ls, bs, ll, lb, w = ref.draw(5, (8,), 1, 70, "rand")
        dl, dll = put(ls[0], dev), put(ll, dev)
        (sims, hint), n = counted(lambda: rocket.distill_losses([dl], [bs[0].to(dev)], dll, lb.to(dev), cosine, w.to(dev)))
        assert n == 1
        g1, g2 = torch.autograd.grad(sims[0] * 0.5 + hint * 1.5, [dl, dll], create_graph=True)
        h1, h2 = torch.autograd.grad(g1.square().sum() + g2.square().sum(), [dl, dll])
        l64, ll64 = ls[0].double().requires_grad_(True), ll.double().requires_grad_(True)
        s64, t64 = rocket.distill_losses_literal([l64], [bs[0].double()], ll64, lb.double(), cosine, w.double())
        k1, k2 = torch.autograd.grad(s64[0] * 0.5 + t64 * 1.5, [l64, ll64], create_graph=True)
        e1, e2 = torch.autograd.grad(k1.square().sum() + k2.square().sum(), [l64, ll64])
        assert torch.allclose(h1.cpu().double(), e1, rtol=1e-4, atol=1e-6) and torch.allclose(h2.cpu().double(), e2, rtol=1e-4, atol=1e-6)


def test_outside_the_limits_and_switched_off_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import rocket

    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    ok = rocket.distill_losses_ok
    assert ok([z(5, 8)], [z(5, 8)], z(5), z(5)) and ok([], [], z(5, 3), z(5, 3)) and ok([z(5, 1024)], [z(5, 1024)], z(5), z(5), z(5))
    assert ok([z(5, 20)[:, 4:12], z(5, 4)], [z(5, 8), z(5, 20)[:, 8:12]], z(5, 64), z(5, 64)) and ok([z(5, 4)] * 8, [z(5, 4)] * 8, z(5), z(5))
    assert not ok([z(5, 6)], [z(5, 6)], z(5), z(5)) and not ok([z(5, 1028)], [z(5, 1028)], z(5), z(5)) and not ok([z(5, 2)], [z(5, 2)], z(5), z(5))
    assert not ok([z(5, 4)] * 9, [z(5, 4)] * 9, z(5), z(5)) and not ok([z(5, 8)], [z(5, 12)], z(5), z(5)) and not ok([z(4, 8)], [z(4, 8)], z(5), z(5))
    assert not ok([], [], z(5, 65), z(5, 65)) and not ok([], [], z(0), z(0)) and not ok([], [], z(5, 2), z(5, 3)) and not ok([], [], z(5, 4)[:, :2], z(5, 2))
    assert not ok([z(5, 8).double()], [z(5, 8).double()], z(5).double(), z(5).double()) and not ok([z(5, 11)[:, :8]], [z(5, 8)], z(5), z(5))
    assert not ok([], [], z(5), z(5), z(4)) and not ok([], [], z(5), z(5), z(5).double()) and not ok([], [], z(5), z(5), z(10)[::2])
    assert not ok([], [], z(5, 2), z(5, 2), z(5))  # ([B, C] * [B] weights: the reference's own broadcast, or its error)
    assert (_lib.DISTILL_MAX_PAIRS, _lib.DISTILL_MAX_W, _lib.DISTILL_MAX_C) == (8, 1024, 64)
    for W, dtype, fused in ((6, torch.float32, True), (8, torch.float64, True), (8, torch.float32, False)):
        monkeypatch.setattr(rocket, "FUSED_DISTILL_LOSS", fused)
        for cosine in (True, False):
            ls, bs, ll, lb, w = ref.draw(5, (W, 4), 1, 80 + W, "rand")
            want = ref.literal(ls, bs, ll, lb, cosine, w)
            gaps = ref.gaps(ls, bs, ll, lb, cosine, w, None, want)
            cast = lambda ts: [t.to(dtype) for t in ts]  # noqa: E731
            got = run(dev, cast(ls), cast(bs), ll.to(dtype), lb.to(dtype), w.to(dtype), cosine, fused=False)
            ref.check(got, want, gaps, f"literal W{W} {dtype} fused={fused} cosine={cosine} on {dev.type}", ref.kinds(2))
