"""match.amm_loss (tzr_amm_loss_fwd / _bwd, csrc/amm_loss.hip): DAT's Adaptive-Mimic loss, both sides in one launch, against the
reference's literal form evaluated in float64 on the CPU (tests/amm_loss_ref.py).  Per kind (loss_u, loss_i, dA_u, dA_i): max |got
- fp64| / max(1, |fp64|) at or below 4 x the distance of torch's own fp32 literal form to the float64 result on the same inputs,
floor 2^-20; no element is left out.  The gradients are taken for the upstream gradients (0.37, -2.0), not 1.

One wave a sample, four samples a workgroup, no loop over the batch: B = 1, 3 (a partial workgroup), 4 (a full one), 5 and 67 (more
than one) are the block shapes there are; the finishing sum's sixteen chains take eight rows a pass, so B = 517 (130 workgroups)
runs their loop twice."""
import pytest
import torch

import amm_loss_ref as ref
from torcheasyrec_amd import _lib

CS = {"half_half": (0.5, 0.5), "zero_u": (0.0, 1.3)}


def put(x, dev, strided=False, grad=True):
    """a leaf on `dev`; strided: the column slice [:, 4 : 4 + D] of a buffer 12 wider"""
    if strided:
        buf = torch.zeros(x.shape[0], x.shape[1] + 12)
        buf[:, 4:4 + x.shape[1]] = x
        return buf.to(dev)[:, 4:4 + x.shape[1]].requires_grad_(grad)
    return x.to(dev).clone().requires_grad_(grad)


def counted(fn):
    """-> (fn's result, the number of tzr_amm_loss_fwd calls it made)"""
    calls, L = [], _lib.lib()
    orig = L.tzr_amm_loss_fwd
    L.tzr_amm_loss_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        return fn(), len(calls)
    finally:
        L.tzr_amm_loss_fwd = orig


def run(dev, ua, ia, ue, ie, w, cosine, c, g=ref.UPSTREAM, strided=False, fused=True):
    from torcheasyrec_amd import match

    dua, dia, due, die = put(ua, dev, strided), put(ia, dev, strided), put(ue, dev, strided), put(ie, dev, strided)
    dw = None if w is None else w.to(dev)
    if fused:
        assert match.FUSED_AMM_LOSS and match.amm_loss_ok(dua, dia, due, die, dw)
    (lu, li), n = counted(lambda: match.amm_loss(dua, dia, due, die, cosine, c[0], c[1], dw))
    assert n == (1 if fused else 0)  # (the kernel, not the literal form -- or the other way round)
    gu, gi, geu, gei = torch.autograd.grad(lu * g[0] + li * g[1], [dua, dia, due, die], allow_unused=True)
    assert geu is None and gei is None  # (the targets are constants)
    return {"loss_u": [lu.detach()], "loss_i": [li.detach()], "dA_u": [gu], "dA_i": [gi]}


def check_case(dev, B, M, D, cosine, weights=None, c=(0.5, 0.5), strided=False, seed=0):
    ua, ia, ue, ie, w = ref.draw(B, M, D, seed, weights)
    want = ref.literal(ua, ia, ue, ie, cosine, c[0], c[1], w)
    gaps = ref.gaps(ua, ia, ue, ie, cosine, c[0], c[1], w, ref.UPSTREAM, want)
    got = run(dev, ua, ia, ue, ie, w, cosine, c, strided=strided)
    ref.check(got, want, gaps, f"B{B} M{M} D{D} cosine={cosine} weights={weights} c={c} strided={strided} on {dev.type}", ref.KINDS)
    tail = got["dA_i"][0][B:]
    assert tail.shape == (M - B, D) and torch.equal(tail.cpu().view(torch.int32), torch.zeros(M - B, D, dtype=torch.int32))  # +0.0, bit for bit
    return got


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("cosine", [True, False])
@pytest.mark.parametrize("negatives", [0, 12])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 67])
def test_every_batch(dev, B, negatives, cosine, weights):
    check_case(dev, B, B + negatives, 8, cosine, weights, seed=B)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("cosine", [True, False])
@pytest.mark.parametrize("D", [4, 8, 60, 64, 252, 256])
def test_every_width_contiguous_and_as_a_column_slice(dev, D, cosine, weights, strided):
    """one float4, two lanes, a lane short of sixteen, sixteen, a lane short of the wave, every lane"""
    check_case(dev, 5, 17, D, cosine, weights, strided=strided, seed=100 + D)


@pytest.mark.parametrize("weights", [None, "rand"])
def test_the_finishing_sums_chains_run_twice(dev, weights):
    check_case(dev, 517, 517 + 12, 8, True, weights, seed=7)


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("cosine", [True, False])
@pytest.mark.parametrize("c", sorted(CS))
def test_the_sides_weights(dev, c, cosine, weights):
    got = check_case(dev, 5, 17, 8, cosine, weights, c=CS[c], seed=20)
    if CS[c][0] == 0.0:
        assert float(got["loss_u"][0]) == 0.0 and float(got["dA_u"][0].abs().max()) == 0.0  # the zero side: exact zeros


@pytest.mark.parametrize("cosine", [True, False])
def test_all_weights_zero(dev, cosine):
    """div_no_nan: losses exactly 0, gradients exactly 0, nothing non-finite"""
    ua, ia, ue, ie, w = ref.draw(5, 17, 8, 30, "zero")
    got = run(dev, ua, ia, ue, ie, w, cosine, (0.5, 0.5))
    for k in ref.KINDS:
        assert bool(torch.isfinite(got[k][0]).all()) and float(got[k][0].abs().max()) == 0.0, k


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("cosine", [True, False])
def test_an_all_zero_augment_row_takes_the_clamp_branch(dev, cosine, weights):
    """F.normalize divides by max(|a|, 1e-12): a zero row has y = 0 and the gradient dy / 1e-12, of the order 1e12 -- checked on that
    row alone so that it does not set the norm for the other rows, and the other rows without it"""
    ua, ia, ue, ie, w = ref.draw(5, 9, 8, 40, weights)
    ua[2] = 0.0
    ia[2] = 0.0
    c = (0.5, 0.5)
    want = ref.literal(ua, ia, ue, ie, cosine, c[0], c[1], w)
    r32 = ref.literal(ua, ia, ue, ie, cosine, c[0], c[1], w, dtype=torch.float32)
    got = run(dev, ua, ia, ue, ie, w, cosine, c)
    assert float(want["dA_u"][0][2].abs().max()) > 1e10 and float(want["dA_i"][0][2].abs().max()) > 1e10  # (the clamp branch)
    for name in ("the zero row", "the other rows"):
        def part(res):
            """the losses whole, of each gradient row 2 alone or every row but it"""
            out = {k: [res[k][0].cpu()] for k in ("loss_u", "loss_i")}
            for k in ("dA_u", "dA_i"):
                t = res[k][0].cpu()
                out[k] = [t[2:3] if name == "the zero row" else torch.cat([t[:2], t[3:]])]
            return out

        w64 = part(want)
        ref.check(part(got), w64, {k: ref.rel_err(part(r32)[k], w64[k]) for k in ref.KINDS},
                  f"{name} cosine={cosine} weights={weights} on {dev.type}", ref.KINDS)


def test_two_runs_are_bit_equal(dev):
    ua, ia, ue, ie, w = ref.draw(67, 79, 64, 50, "rand")
    a, b = run(dev, ua, ia, ue, ie, w, True, (0.5, 0.5)), run(dev, ua, ia, ue, ie, w, True, (0.5, 0.5))
    for k in ref.KINDS:
        assert torch.equal(a[k][0], b[k][0]), k


def test_one_side_alone_gets_its_gradient(dev):
    """a loss nobody differentiates hands the backward no gradient: that side's rows are zeros, the other side's as before"""
    from torcheasyrec_amd import match

    ua, ia, ue, ie, _ = ref.draw(5, 9, 8, 60)
    both = run(dev, ua, ia, ue, ie, None, True, (0.5, 0.5), g=(0.37, 0.0))
    dua, dia = put(ua, dev), put(ia, dev)
    lu, _ = match.amm_loss(dua, dia, ue.to(dev), ie.to(dev), True, 0.5, 0.5)
    gu, gi = torch.autograd.grad(lu * 0.37, [dua, dia])
    assert torch.equal(gu, both["dA_u"][0]) and float(gi.abs().max()) == 0.0


def test_a_double_backward_goes_through_the_literal_form(dev):
    from torcheasyrec_amd import match

    ua, ia, ue, ie, w = ref.draw(5, 9, 8, 70, "rand")
    dua, dia = put(ua, dev), put(ia, dev)
    (lu, li), n = counted(lambda: match.amm_loss(dua, dia, ue.to(dev), ie.to(dev), True, 0.5, 0.5, w.to(dev)))
    assert n == 1
    gu, gi = torch.autograd.grad(lu + li, [dua, dia], create_graph=True)
    hu, = torch.autograd.grad(gu.square().sum() + gi.square().sum(), [dua])
    a64, i64 = ua.double().requires_grad_(True), ia.double().requires_grad_(True)
    l64 = match.amm_loss_literal(a64, i64, ue.double(), ie.double(), True, 0.5, 0.5, w.double())
    g64 = torch.autograd.grad(l64[0] + l64[1], [a64, i64], create_graph=True)
    h64, = torch.autograd.grad(g64[0].square().sum() + g64[1].square().sum(), [a64])
    assert torch.allclose(hu.cpu().double(), h64, rtol=1e-4, atol=1e-6)


def test_outside_the_limits_and_switched_off_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import match

    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    ok = match.amm_loss_ok
    assert ok(z(5, 8), z(9, 8), z(5, 8), z(9, 8)) and ok(z(5, 256), z(5, 256), z(5, 256), z(5, 256)) and ok(z(5, 8), z(9, 8), z(5, 8), z(9, 8), z(5))
    assert ok(z(5, 20)[:, 4:12], z(9, 8), z(5, 8), z(9, 20)[:, 4:12])
    assert not ok(z(5, 6), z(9, 6), z(5, 6), z(9, 6)) and not ok(z(5, 260), z(9, 260), z(5, 260), z(9, 260)) and not ok(z(5, 2), z(9, 2), z(5, 2), z(9, 2))
    assert not ok(z(5, 8), z(4, 8), z(5, 8), z(4, 8)) and not ok(z(0, 8), z(4, 8), z(0, 8), z(4, 8)) and not ok(z(5, 8), z(9, 8), z(5, 8), z(8, 8))
    assert not ok(z(5, 8).double(), z(9, 8).double(), z(5, 8).double(), z(9, 8).double()) and not ok(z(5, 11)[:, :8], z(9, 8), z(5, 8), z(9, 8))
    assert not ok(z(5, 8), z(9, 8), z(5, 8), z(9, 8), z(4)) and not ok(z(5, 8), z(9, 8), z(5, 8), z(9, 8), z(5).double())
    assert _lib.AMM_MAX_D == 256
    for D, dtype, fused in ((6, torch.float32, True), (260, torch.float32, True), (8, torch.float64, True), (8, torch.float32, False)):
        monkeypatch.setattr(match, "FUSED_AMM_LOSS", fused)
        ua, ia, ue, ie, w = (None if t is None else t.to(dtype) for t in ref.draw(5, 9, D, 80 + D, "rand"))
        want = ref.literal(ua, ia, ue, ie, True, 0.5, 0.5, w)
        gaps = ref.gaps(ua.float(), ia.float(), ue.float(), ie.float(), True, 0.5, 0.5, w.float(), ref.UPSTREAM, want)
        got = run(dev, ua, ia, ue, ie, w, True, (0.5, 0.5), fused=False)
        ref.check(got, want, gaps, f"literal D{D} {dtype} fused={fused} on {dev.type}", ref.KINDS)
