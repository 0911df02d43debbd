"""match.label_attention (tzr_label_attn_fwd / _bwd, csrc/label_attention.hip): MIND's label-aware attention against the
reference's literal form evaluated in float64 on the CPU (tests/capsule_ref.py).  Per kind (user_emb, w, dI, dV): max |got - fp64|
/ max(1, |fp64|) at or below 4 x the literal fp32 form's own distance to the float64 result on the same inputs, floor 2^-20; no
element is left out.  One wave a sample, four samples a workgroup, no loop over the batch: B = 1, 5 (a partial workgroup) and 65
(seventeen workgroups) are the block shapes there are."""
import pytest
import torch

import capsule_ref as ref
from torcheasyrec_amd import _lib


def put3(x, dev, strided=False):
    """[B, K, D] leaf on `dev`; strided: the column slice [:, 4 : 4 + D] of a [B K, D + 12] buffer"""
    if strided:
        B, K, D = x.shape
        buf = torch.zeros(B * K, D + 12)
        buf[:, 4:4 + D] = x.reshape(B * K, D)
        return buf.to(dev)[:, 4:4 + D].unflatten(0, (B, K)).requires_grad_(True)
    return x.to(dev).clone().requires_grad_(True)


def put2(x, dev, strided=False):
    if strided:
        buf = torch.zeros(x.shape[0], x.shape[1] + 12)
        buf[:, 4:4 + x.shape[1]] = x
        return buf.to(dev)[:, 4:4 + x.shape[1]].requires_grad_(True)
    return x.to(dev).clone().requires_grad_(True)


def run(dev, interests, item, mask, simi_pow, g, strided=False):
    from torcheasyrec_amd import match

    di, dv, dm = put3(interests, dev, strided), put2(item, dev, strided), mask.to(dev)
    assert match.FUSED_LABEL_ATTENTION and match.label_attention_ok(di, dv, dm, simi_pow)
    calls = []
    L = _lib.lib()
    orig = L.tzr_label_attn_fwd
    L.tzr_label_attn_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        emb, w = match.label_attention(di, dv, dm, simi_pow, want_weights=True)
    finally:
        L.tzr_label_attn_fwd = orig
    assert calls == [1]  # (the kernel, not the literal form)
    gi, gv = torch.autograd.grad((emb * g.to(dev)).sum(), [di, dv])
    return {"user_emb": [emb.detach()], "w": [w], "dI": [gi], "dV": [gv]}


def check_case(dev, B, K, D, valid, simi_pow, M=None, strided=False, seed=0):
    interests, item, mask, g = ref.la_draw(B, K, D, B + 3 if M is None else M, valid, seed)
    want = ref.la_literal(interests, item, mask, simi_pow, g)
    gaps = ref.la_gaps(interests, item, mask, simi_pow, g, want)
    got = run(dev, interests, item, mask, simi_pow, g, strided)
    ref.check(got, want, gaps, f"B{B} K{K} D{D} {valid} simi_pow{simi_pow} strided={strided} on {dev.type}", ref.LA_KINDS)
    assert float(got["w"][0][~mask.to(dev)].abs().sum()) == 0.0 and float(got["dI"][0][~mask.to(dev)].abs().sum()) == 0.0  # exactly zero
    assert float(got["dV"][0][B:].abs().sum()) == 0.0  # (only the positives attend)
    return got


@pytest.mark.parametrize("simi_pow", [1.0, 10.0])
@pytest.mark.parametrize("valid", ["one", "some", "all"])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_every_capsule_count_and_mask(dev, K, valid, simi_pow):
    check_case(dev, 5, K, 8, valid, simi_pow, seed=K)


@pytest.mark.parametrize("simi_pow", [1.0, 10.0])
@pytest.mark.parametrize("D", [4, 8, 64, 256])
def test_every_width(dev, D, simi_pow):
    """one float4, two lanes, sixteen, every lane of the wave"""
    check_case(dev, 5, 3, D, "some", simi_pow, seed=10 + D)


@pytest.mark.parametrize("simi_pow", [1.0, 10.0])
@pytest.mark.parametrize("B", [1, 5, 65])
def test_every_batch(dev, B, simi_pow):
    check_case(dev, B, 3, 8, "some", simi_pow, seed=20 + B)


@pytest.mark.parametrize("simi_pow", [1.0, 10.0])
def test_no_item_rows_behind_the_positives(dev, simi_pow):
    check_case(dev, 5, 3, 8, "some", simi_pow, M=5, seed=30)


@pytest.mark.parametrize("simi_pow", [1.0, 10.0])
def test_interests_and_items_as_column_slices(dev, simi_pow):
    check_case(dev, 5, 3, 12, "some", simi_pow, strided=True, seed=40)


def test_two_runs_are_bit_equal(dev):
    interests, item, mask, g = ref.la_draw(65, 8, 64, 70, "some", 50)
    a, b = run(dev, interests, item, mask, 10.0, g), run(dev, interests, item, mask, 10.0, g)
    for k in ref.LA_KINDS:
        assert torch.equal(a[k][0], b[k][0]), k


def test_outside_the_limits_and_switched_off_the_literal_form_runs(dev, monkeypatch):
    from torcheasyrec_amd import match

    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    mk = lambda B, K: torch.ones(B, K, dtype=torch.bool, device=dev)  # noqa: E731
    ok = match.label_attention_ok
    assert ok(z(5, 3, 8), z(9, 8), mk(5, 3), 1.0) and ok(z(5, 8, 256), z(5, 256), mk(5, 8), 10.0)
    assert not ok(z(5, 3, 6), z(9, 6), mk(5, 3), 1.0) and not ok(z(5, 3, 260), z(9, 260), mk(5, 3), 1.0) and not ok(z(5, 9, 8), z(9, 8), mk(5, 9), 1.0)
    assert not ok(z(5, 3, 8), z(4, 8), mk(5, 3), 1.0) and not ok(z(5, 3, 8), z(9, 8), mk(5, 3), 0.0) and not ok(z(5, 3, 8), z(9, 8), mk(5, 3).float(), 1.0)
    assert not ok(z(5, 3, 8).double(), z(9, 8).double(), mk(5, 3), 1.0) and not ok(z(5, 3, 11)[:, :, :8], z(9, 8), mk(5, 3), 1.0)
    assert (_lib.LABEL_ATTN_MAX_D, _lib.LABEL_ATTN_MAX_K) == (256, 8)
    calls = []
    L = _lib.lib()
    orig = L.tzr_label_attn_fwd
    L.tzr_label_attn_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        for D, fused in ((6, True), (8, False)):
            monkeypatch.setattr(match, "FUSED_LABEL_ATTENTION", fused)
            interests, item, mask, g = ref.la_draw(5, 3, D, 8, "some", 60 + D)
            want = ref.la_literal(interests, item, mask, 10.0, g)
            gaps = ref.la_gaps(interests, item, mask, 10.0, g, want)
            di, dv = put3(interests, dev), put2(item, dev)
            emb, w = match.label_attention(di, dv, mask.to(dev), 10.0, want_weights=True)
            gi, gv = torch.autograd.grad((emb * g.to(dev)).sum(), [di, dv])
            ref.check({"user_emb": [emb.detach()], "w": [w], "dI": [gi], "dV": [gv]}, want, gaps, f"literal D{D}", ref.LA_KINDS)
    finally:
        L.tzr_label_attn_fwd = orig
    assert calls == []


def test_the_entry_points_refuse_by_code(dev):
    """null and misaligned rows, every limit exceeded by one; nothing is written"""
    L = _lib.lib()
    B, K, D = 5, 3, 8
    f = lambda *s: torch.full(s, 12345.0, dtype=torch.float32, device=dev)  # noqa: E731
    i, v, g, out, w, di, dv = f(B * K, D), f(B, D), f(B, D), f(B, D), f(B, K), f(B * K, D), f(B, D)
    mask = torch.ones(B, K, dtype=torch.bool, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731

    def fwd(i_=p(i), is_=D, v_=p(v), vs=D, m_=p(mask), b=B, k=K, d=D, sp=1.0, o_=p(out), os_=D, w_=p(w)):
        return L.tzr_label_attn_fwd(i_, is_, v_, vs, m_, b, k, d, sp, o_, os_, w_, None)

    def bwd(g_=p(g), gs=D, i_=p(i), is_=D, v_=p(v), vs=D, w_=p(w), m_=p(mask), b=B, k=K, d=D, sp=1.0, di_=p(di), dis=D, dv_=p(dv), dvs=D):
        return L.tzr_label_attn_bwd(g_, gs, i_, is_, v_, vs, w_, m_, b, k, d, sp, di_, dis, dv_, dvs, None)

    INVALID, UNSUPPORTED = -1, -4
    for kw, code in ((dict(d=6), UNSUPPORTED), (dict(d=0), UNSUPPORTED), (dict(d=260), UNSUPPORTED), (dict(k=0), UNSUPPORTED), (dict(k=9), UNSUPPORTED),
                     (dict(sp=0.0), UNSUPPORTED), (dict(is_=9), UNSUPPORTED), (dict(vs=4), UNSUPPORTED), (dict(b=-1), INVALID), (dict(i_=None), INVALID),
                     (dict(v_=p(v) + 4), INVALID), (dict(m_=None), INVALID), (dict(w_=None), INVALID)):
        assert fwd(**kw) == code and bwd(**kw) == code, kw
    for kw, code in ((dict(o_=None), INVALID), (dict(o_=p(out) + 4), INVALID), (dict(os_=4), UNSUPPORTED)):
        assert fwd(**kw) == code, kw
    for kw, code in ((dict(g_=None), INVALID), (dict(gs=9), UNSUPPORTED), (dict(di_=None), INVALID), (dict(dis=4), UNSUPPORTED), (dict(dv_=p(dv) + 4), INVALID),
                     (dict(dvs=9), UNSUPPORTED)):
        assert bwd(**kw) == code, kw
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for t in (out, w, di, dv):
        assert bool((t == 12345.0).all())
    assert fwd(b=0) == 0 and bwd(b=0) == 0 and bool((out == 12345.0).all())
    for name in ("tzr_label_attn_fwd", "tzr_label_attn_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS
