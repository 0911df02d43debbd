"""Error behaviour of the four tzr_jagged_* entry points (csrc/jagged_encoders.hip), as tests/test_abi_errors.py checks their
siblings: bad arguments come back as negative status codes -- never a crash, never a launch -- and B == 0 is a TZR_OK no-op."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from torcheasyrec_amd import _lib  # noqa: E402

OK, INVALID, UNSUPPORTED = 0, -1, -4
D, B, N = 8, 2, 5


def _bufs(dev):
    kv, q, out, pr, dkv, dq = (torch.zeros(n + 4, dtype=torch.float32, device=dev) for n in (N * D, B * D, B * D, N, N * D, B * D))
    return kv, q, out, pr, dkv, dq, torch.tensor([0, 2, 5], dtype=torch.int64, device=dev)


def test_dot_attention_rejects_bad_arguments(dev):
    L, p = _lib.lib(), _lib.ptr
    kv, q, out, pr, dkv, dq, off = _bufs(dev)

    def fwd(kv_=p(kv), kvs=D, q_=p(q), qs=D, d=D, off_=p(off), b=B, n=N, ml=4, out_=p(out), outs=D, p_=p(pr)):
        return L.tzr_jagged_dot_attn_fwd(kv_, kvs, q_, qs, d, off_, b, n, ml, out_, outs, p_, None)

    def bwd(g_=p(out), gs=D, p_=p(pr), kv_=p(kv), kvs=D, q_=p(q), qs=D, d=D, off_=p(off), b=B, n=N, ml=4, dkv_=p(dkv), dks=D, dq_=p(dq),
            dqs=D):
        return L.tzr_jagged_dot_attn_bwd(g_, gs, p_, kv_, kvs, q_, qs, d, off_, b, n, ml, dkv_, dks, dq_, dqs, None)

    assert fwd() == OK and bwd() == OK
    for fn, names in ((fwd, ("kv_", "q_", "off_", "out_", "p_")), (bwd, ("g_", "p_", "kv_", "q_", "off_", "dkv_", "dq_"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name  # null pointer
        assert fn(b=-1) == INVALID and fn(n=-1) == INVALID and fn(ml=-1) == INVALID and fn(d=0) == INVALID
        assert fn(d=6) == UNSUPPORTED  # D % 4
        assert fn(d=260, kvs=260, qs=260) == UNSUPPORTED  # more than one lane per float4 piece of a row
        assert fn(kvs=10) == UNSUPPORTED and fn(qs=10) == UNSUPPORTED  # stride no multiple of 4 floats
        assert fn(kvs=4) == UNSUPPORTED  # stride below D
        assert fn(ml=2049) == UNSUPPORTED  # a sample's scores live in LDS
        assert fn(kv_=p(kv) + 4) == INVALID  # 16-byte alignment
        assert fn(b=0, off_=None, q_=None) == OK  # no sample: nothing to do
    assert fwd(outs=10) == UNSUPPORTED and bwd(dks=10) == UNSUPPORTED and bwd(dqs=10) == UNSUPPORTED and bwd(gs=10) == UNSUPPORTED
    assert fwd(out_=p(out) + 4) == INVALID and bwd(dq_=p(dq) + 4) == INVALID
    # no row at all: no row pointer needed, the outputs are zero rows
    off0 = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    out.fill_(1.0)
    assert fwd(kv_=None, p_=None, n=0, off_=p(off0)) == OK and bwd(kv_=None, p_=None, dkv_=None, n=0, off_=p(off0)) == OK
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert float(out[:B * D].abs().sum()) == 0.0


def test_pooling_rejects_bad_arguments(dev):
    L, p = _lib.lib(), _lib.ptr
    kv, q, out, pr, dkv, dq, off = _bufs(dev)

    def fwd(kv_=p(kv), kvs=D, d=D, off_=p(off), b=B, n=N, ml=4, mode=1, out_=p(out), outs=D):
        return L.tzr_jagged_pool_fwd(kv_, kvs, d, off_, b, n, ml, mode, out_, outs, None)

    def bwd(g_=p(out), gs=D, d=D, off_=p(off), b=B, n=N, ml=4, mode=1, dkv_=p(dkv), dks=D):
        return L.tzr_jagged_pool_bwd(g_, gs, d, off_, b, n, ml, mode, dkv_, dks, None)

    assert fwd() == OK and bwd() == OK and fwd(mode=0) == OK and bwd(mode=0) == OK
    for fn, names in ((fwd, ("kv_", "off_", "out_")), (bwd, ("g_", "off_", "dkv_"))):
        for name in names:
            assert fn(**{name: None}) == INVALID, name
        assert fn(b=-1) == INVALID and fn(n=-1) == INVALID and fn(ml=-1) == INVALID and fn(d=0) == INVALID and fn(mode=2) == INVALID
        assert fn(d=6) == UNSUPPORTED and fn(d=260) == UNSUPPORTED
        assert fn(b=0, off_=None) == OK
    assert fwd(kvs=10) == UNSUPPORTED and fwd(outs=10) == UNSUPPORTED and fwd(kvs=4) == UNSUPPORTED
    assert bwd(gs=10) == UNSUPPORTED and bwd(dks=10) == UNSUPPORTED
    assert fwd(kv_=p(kv) + 4) == INVALID and fwd(out_=p(out) + 4) == INVALID and bwd(dkv_=p(dkv) + 4) == INVALID
    off0 = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    assert fwd(kv_=None, n=0, off_=p(off0)) == OK and bwd(dkv_=None, n=0, off_=p(off0)) == OK
