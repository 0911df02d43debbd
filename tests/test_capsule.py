"""capsule.capsule_routing (tzr_capsule_fwd / _bwd, csrc/capsule_routing.hip): MIND's behaviour-to-interest capsule layer on
jagged rows, against the reference's padded form evaluated in float64 on the CPU (tests/capsule_ref.py).  Per kind (high, c, dX,
dW): max |got - fp64| / max(1, |fp64|) at or below 4 x the literal fp32 form's own distance to the float64 result on the same
inputs (the larger of two evaluations, as given and with each sample's positions reversed), floor 2^-20; no element is left out.
`mask` equals the integer rule exactly.  Every case runs in both settings: the reference test's (scale 1, stddev 0.1, pow 2) and
the defaults (scale 20, stddev 1, pow 1).

One axis at a time around B = 9, S = 20, L = 16, H = 8, K = 4, 3 iterations.  The backward's grid is capped
(_lib.CAPSULE_BWD_MAX_GRID): `test_one_sample_more_than_the_backward_grid` makes one workgroup walk two samples and the
finishing launch add more than one round of partial rows."""
import ctypes as C

import pytest
import torch

import capsule_ref as ref
from torcheasyrec_amd import _lib

BASE_LENGTHS = [0, 1, 2, 5, 17, 20, 23, 3, 16]
SETTINGS = sorted(ref.SETTINGS)
MAX_DRAWS = 8


def put(x, dev, strided=False):
    """a leaf on `dev`; strided: the column slice [:, 4 : 4 + L] of a buffer 12 wider"""
    if strided:
        buf = torch.zeros(x.shape[0], x.shape[1] + 12)
        buf[:, 4:4 + x.shape[1]] = x
        return buf.to(dev)[:, 4:4 + x.shape[1]].requires_grad_(True)
    return x.to(dev).clone().requires_grad_(True)


def settled(lengths, cfg, L, seed, with_logits0=True):
    """inputs, the float64 result and the yardstick; the seed steps by 1000 until the literal fp32 routing weights stay within
    ref.C_YARDSTICK_MAX of float64 (a condition on the inputs, checked with the reference alone)"""
    for n in range(MAX_DRAWS):
        offsets, x, W, l0, g = ref.draw(lengths, L, cfg.high_dim, cfg.max_k, seed + 1000 * n, with_logits0)
        want = ref.literal(x, offsets, W, cfg, l0, g, torch.float64)
        try:
            return (offsets, x, W, l0, g), want, ref.gaps(x, offsets, W, cfg, l0, g, want)
        except AssertionError:
            continue
    raise AssertionError(f"no settled draw within {MAX_DRAWS} draws at lengths {lengths}")


def run(dev, inputs, cfg, strided=False):
    from torcheasyrec_amd import capsule

    offsets, x, W, l0, g = inputs
    ccfg = capsule.CapsuleConfig(**vars(cfg))
    dx, dw, doff = put(x, dev, strided), put(W, dev), offsets.to(dev)
    dl0 = None if l0 is None else l0.to(dev)
    assert capsule.FUSED_CAPSULE and capsule.capsule_ok(dx, doff, dw, ccfg, dl0)
    calls = []
    L = _lib.lib()
    orig = L.tzr_capsule_fwd
    L.tzr_capsule_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        high, mask = capsule.capsule_routing(dx, doff, dw, ccfg, dl0)
    finally:
        L.tzr_capsule_fwd = orig
    assert calls == [1]  # (the kernel, not the literal form)
    gx, gw = torch.autograd.grad((high * g.to(dev)).sum(), [dx, dw])
    high2, mask2, c = capsule._CapsuleFn.apply(dx, doff, dw, dl0, ccfg)  # (the routing weights are the Function's third output)
    assert torch.equal(high2, high) and torch.equal(mask2, mask)
    return {"high": [high.detach()], "c": [c], "dX": [gx], "dW": [gw], "mask": mask}


def check_case(dev, setting, lengths=BASE_LENGTHS, S=20, L=16, H=8, K=4, iters=3, const_caps_num=False, with_logits0=True,
               strided=False, seed=0):
    cfg = ref.config(S=S, K=K, H=H, iters=iters, const_caps_num=const_caps_num, **ref.SETTINGS[setting])
    inputs, want, gaps = settled(lengths, cfg, L, seed, with_logits0)
    got = run(dev, inputs, cfg, strided)
    what = f"{setting} B{len(lengths)} S{S} L{L} H{H} K{K} iters{iters} const={const_caps_num} logits0={with_logits0} strided={strided} on {dev.type}"
    ref.check(got, want, gaps, what, ref.KINDS)
    assert got["mask"].dtype == torch.bool and torch.equal(got["mask"].cpu(), want["mask"]), f"{what}: mask against the float form"
    assert torch.equal(got["mask"].cpu(), ref.integer_mask(lengths, K, const_caps_num)), f"{what}: mask against the integer rule"
    high = got["high"][0].cpu()
    assert float(high[~want["mask"]].abs().max() if (~want["mask"]).any() else 0.0) == 0.0, f"{what}: masked capsules are zeros"
    return got, want, inputs


@pytest.mark.parametrize("setting", SETTINGS)
def test_every_length_in_one_batch(dev, setting):
    """powers of two (the capsule count steps behind them), the 16-row tile's tails, truncation at S = 20 with k_b from the
    untruncated length"""
    check_case(dev, setting, lengths=[0, 1, 2, 3, 4, 5, 15, 16, 17, 19, 20, 23], seed=1)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("S", [16, 40])
def test_every_max_seq_len(dev, S, setting):
    check_case(dev, setting, lengths=[0, 1, 2, 5, 17, 20, 23, 40, 45], S=S, seed=10 + S)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_every_capsule_count(dev, K, setting):
    check_case(dev, setting, K=K, seed=20 + K)


@pytest.mark.parametrize("setting", SETTINGS)
def test_const_caps_num(dev, setting):
    check_case(dev, setting, const_caps_num=True, seed=30)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("L", [4, 20, 128])
def test_every_low_dim(dev, L, setting):
    check_case(dev, setting, L=L, seed=40 + L)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("H", [4, 12, 64, 128])
def test_every_high_dim(dev, H, setting):
    check_case(dev, setting, H=H, seed=50 + H)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("iters", [1, 2, 8])
def test_every_iteration_count(dev, iters, setting):
    check_case(dev, setting, iters=iters, seed=60 + iters)


@pytest.mark.parametrize("setting", SETTINGS)
def test_logits0_null(dev, setting):
    check_case(dev, setting, with_logits0=False, seed=70)


@pytest.mark.parametrize("setting", SETTINGS)
def test_x_as_a_column_slice_of_a_wider_buffer(dev, setting):
    check_case(dev, setting, strided=True, seed=80)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("length", [0, 7])
def test_one_sample(dev, length, setting):
    check_case(dev, setting, lengths=[length], seed=90 + length)


@pytest.mark.parametrize("setting", SETTINGS)
def test_one_sample_more_than_the_backward_grid(dev, setting):
    """B = the cap + 1: workgroup 0 walks two samples, and the finishing launch's sixteen chains take more than one row each"""
    B = _lib.CAPSULE_BWD_MAX_GRID + 1
    check_case(dev, setting, lengths=[(3 * i) % 7 for i in range(B)], S=4, L=4, H=4, K=2, seed=100)


@pytest.mark.parametrize("setting", SETTINGS)
def test_high_into_a_column_slice(dev, setting):
    """`high` with a row stride above its width, through the C entry point"""
    cfg = ref.config(**ref.SETTINGS[setting])
    (offsets, x, W, l0, g), want, gaps = settled(BASE_LENGTHS, cfg, 16, 110)
    B, K, H, N = len(BASE_LENGTHS), cfg.max_k, cfg.high_dim, x.shape[0]
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    wide, pre, c = f(B * K, H + 12), f(B, K, H), f(N, K)
    mask = torch.zeros(B, K, dtype=torch.bool, device=dev)
    dx, dW, doff, dl0 = x.to(dev), W.to(dev), offsets.to(dev), l0.to(dev)
    m = _lib.TzrCapsule()
    m.B, m.N, m.L, m.H, m.K, m.S, m.num_iters = B, N, 16, H, K, cfg.max_seq_len, cfg.num_iters
    m.scale, m.stddev, m.squash_pow = cfg.routing_logits_scale, cfg.routing_logits_stddev, cfg.squash_pow
    m.x, m.x_stride, m.offsets, m.w, m.logits0 = dx.data_ptr(), 16, doff.data_ptr(), dW.data_ptr(), dl0.data_ptr()
    m.high, m.high_stride, m.mask, m.c, m.pre = wide[:, 4:].data_ptr(), wide.stride(0), mask.data_ptr(), c.data_ptr(), pre.data_ptr()
    assert _lib.lib().tzr_capsule_fwd(C.byref(m), _lib.stream_ptr(dev)) == 0
    got = {"high": [wide[:, 4:4 + H].reshape(B, K, H)], "c": [c]}
    ref.check(got, want, gaps, f"strided high {setting} on {dev.type}", ("high", "c"))
    assert bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 4 + H:]).all())  # (nothing outside the slice)
    assert torch.equal(mask.cpu(), want["mask"])


@pytest.mark.parametrize("setting", SETTINGS)
def test_two_runs_are_bit_equal_and_rows_behind_S_get_zero_gradients(dev, setting):
    cfg = ref.config(**ref.SETTINGS[setting])
    lengths = [23, 0, 40, 20, 21]
    inputs, want, _ = settled(lengths, cfg, 16, 120)
    a, b = run(dev, inputs, cfg), run(dev, inputs, cfg)
    for k in ref.KINDS:
        assert torch.equal(a[k][0], b[k][0]), k
    offsets = inputs[0].tolist()
    for i, n in enumerate(lengths):
        behind = slice(offsets[i] + min(n, 20), offsets[i + 1])
        assert float(a["dX"][0][behind].abs().sum()) == 0.0 and float(a["c"][0][behind].abs().sum()) == 0.0
        assert float(want["dX"][0][behind].abs().sum()) == 0.0


def test_an_upstream_gradient_scales_both_gradients(dev):
    from torcheasyrec_amd import capsule

    cfg = ref.config(**ref.SETTINGS["scale1_std0.1_pow2"])
    offsets, x, W, l0, g = ref.draw(BASE_LENGTHS, 16, 8, 4, 130)
    dx, dw = put(x, dev), put(W, dev)
    high, _ = capsule.capsule_routing(dx, offsets.to(dev), dw, capsule.CapsuleConfig(**vars(cfg)), l0.to(dev))
    loss = (high * g.to(dev)).sum()
    g1 = torch.autograd.grad(loss, [dx, dw], retain_graph=True)
    g2 = torch.autograd.grad(loss * 0.25, [dx, dw])
    for p, q in zip(g1, g2):
        assert torch.allclose(p * 0.25, q, rtol=1e-5, atol=1e-8)


def test_outside_the_limits_the_literal_form_runs(dev):
    from torcheasyrec_amd import capsule

    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    off = torch.tensor([0, 3, 5], device=dev)
    cc = lambda **kw: capsule.CapsuleConfig(**{**dict(max_k=4, max_seq_len=20, high_dim=8), **kw})  # noqa: E731
    ok = capsule.capsule_ok
    assert ok(z(5, 16), off, z(16, 8), cc()) and ok(z(5, 128), off, z(128, 128), cc(max_seq_len=64)) and ok(z(5, 4), off, z(4, 64), cc(max_seq_len=128))
    assert ok(z(5, 16), off, z(16, 8), cc(max_k=8, num_iters=8), z(5, 8))
    assert not ok(z(5, 6), off, z(6, 8), cc()) and not ok(z(5, 132), off, z(132, 8), cc()) and not ok(z(5, 16), off, z(16, 6), cc())
    assert not ok(z(5, 16), off, z(16, 132), cc()) and not ok(z(5, 16), off, z(16, 8), cc(max_k=9)) and not ok(z(5, 16), off, z(16, 8), cc(num_iters=9))
    assert not ok(z(5, 16), off, z(16, 8), cc(max_seq_len=129)) and not ok(z(5, 16), off, z(16, 128), cc(max_seq_len=65))
    assert not ok(z(5, 16), off, z(16, 68), cc(max_seq_len=128)) and not ok(z(5, 16), off, z(16, 8), cc(routing_logits_scale=0.0))
    assert not ok(z(5, 16).double(), off, z(16, 8).double(), cc()) and not ok(z(5, 19)[:, :16], off, z(16, 8), cc())
    assert not ok(z(5, 16), off.int(), z(16, 8), cc()) and not ok(z(5, 16), off, z(16, 8), cc(), z(4, 4))
    assert (_lib.CAPSULE_MAX_DIM, _lib.CAPSULE_MAX_K, _lib.CAPSULE_MAX_ITERS, _lib.CAPSULE_MAX_S, _lib.CAPSULE_MAX_SH) == (128, 8, 8, 128, 8192)
    # L = 6: the literal form, the same numbers, and the entry point is never called
    cfg = ref.config(**ref.SETTINGS["scale1_std0.1_pow2"])
    offsets, x, W, l0, g = ref.draw(BASE_LENGTHS, 6, 8, 4, 140)
    want = ref.literal(x, offsets, W, cfg, l0, g, torch.float64)
    gaps = ref.gaps(x, offsets, W, cfg, l0, g, want)
    calls = []
    L = _lib.lib()
    orig = L.tzr_capsule_fwd
    L.tzr_capsule_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        dx, dw = put(x, dev), put(W, dev)
        high, mask = capsule.capsule_routing(dx, offsets.to(dev), dw, capsule.CapsuleConfig(**vars(cfg)), l0.to(dev))
    finally:
        L.tzr_capsule_fwd = orig
    assert calls == []
    gx, gw = torch.autograd.grad((high * g.to(dev)).sum(), [dx, dw])
    ref.check({"high": [high.detach()], "dX": [gx], "dW": [gw]}, want, gaps, "literal L6", ("high", "dX", "dW"))
    assert torch.equal(mask.cpu(), want["mask"])


def test_fused_off_runs_the_literal_form(dev, monkeypatch):
    from torcheasyrec_amd import capsule

    monkeypatch.setattr(capsule, "FUSED_CAPSULE", False)
    cfg = ref.config(**ref.SETTINGS["scale20_std1_pow1"])
    (offsets, x, W, l0, g), want, gaps = settled(BASE_LENGTHS, cfg, 16, 150)
    dx, dw = put(x, dev), put(W, dev)
    high, mask = capsule.capsule_routing(dx, offsets.to(dev), dw, capsule.CapsuleConfig(**vars(cfg)), l0.to(dev))
    gx, gw = torch.autograd.grad((high * g.to(dev)).sum(), [dx, dw])
    ref.check({"high": [high.detach()], "dX": [gx], "dW": [gw]}, want, gaps, "literal", ("high", "dX", "dW"))
    assert torch.equal(mask.cpu(), want["mask"])


@pytest.mark.parametrize("init", ["normal", "zeros"])
def test_the_layer_draws_its_logits_on_the_device(dev, init, monkeypatch):
    """CapsuleLayer: the reference's parameter name, `normal` passes a [N, K] draw on, `zeros` none"""
    from torcheasyrec_amd import capsule

    torch.manual_seed(0)
    layer = capsule.CapsuleLayer(capsule.CapsuleConfig(max_k=4, max_seq_len=20, high_dim=8, routing_init_method=init), 16, device=dev)
    assert [n for n, _ in layer.named_parameters()] == ["bilinear_matrix"] and layer.bilinear_matrix.shape == (16, 8)
    offsets, x, _, _, _ = ref.draw(BASE_LENGTHS, 16, 8, 4, 160)
    seen = []
    orig = capsule.capsule_routing
    monkeypatch.setattr(capsule, "capsule_routing", lambda *a: (seen.append(a[4]), orig(*a))[1])
    high, mask = layer(x.to(dev), offsets.to(dev))
    assert len(seen) == 1 and (seen[0] is not None) == (init == "normal") and (seen[0] is None or seen[0].shape == (x.shape[0], 4))
    assert high.shape == (9, 4, 8) and torch.equal(mask.cpu(), ref.integer_mask(BASE_LENGTHS, 4, False))
    high.sum().backward()
    assert layer.bilinear_matrix.grad is not None and bool(torch.isfinite(layer.bilinear_matrix.grad).all())
    with pytest.raises(ValueError, match="routing_init_method"):
        capsule.CapsuleLayer(capsule.CapsuleConfig(routing_init_method="uniform"), 16)
