"""W1 of the fused interaction layer in fragment order (csrc/interaction_pack.h): the packed prologues load the same numbers into
the same registers as the staged ones, so every output is BIT-identical to the plain entry points; the dense optimizer's
launch writes the copies the pack kernel would; a W1 overwritten behind the optimizer's back is packed again before its use."""
import pytest
import torch

from torcheasyrec_amd import _lib

D, F, H = 16, 26, 64
WIDTH = 27 * 26 // 2 + 27 * D


def _inputs(dev, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    return r(B, D), r(B, F * D), r(H, WIDTH) * 0.05, r(H), r(B, H)


# one partial tile; exactly one tile; a tile and one sample; more tiles than workgroups with a ragged end (257 x 16 + 1)
@pytest.mark.parametrize("B", [1, 16, 17, 4113])
@pytest.mark.parametrize("scaled", [False, True])
def test_packed_prologues_bit_identical(dev, B, scaled):
    from torcheasyrec_amd.dense import pack_w1

    L = _lib.lib()
    if dev.type == "cpu" and B == 4113:  # the lane emulator: the same case (more tiles than workgroups, ragged end) at 2 workgroups
        B = 4 * 16 + 1
        L.tzr_tune(b"it_wgs", 2)
    dense, sparse, W1, b1, g1 = _inputs(dev, B)
    scale = torch.full((1,), 0.37, device=dev) if scaled else None
    fwd_p, bwd_p = pack_w1(W1)
    st = _lib.stream_ptr(dev)
    out = {}
    for name, pf, pb in (("plain", None, None), ("packed", fwd_p, bwd_p)):
        y1 = torch.full((B, H), float("nan"), device=dev)
        gd, gs = torch.full_like(dense, float("nan")), torch.full_like(sparse, float("nan"))
        _lib.check(L.tzr_dot_interaction_top_fwd_packed(_lib.ptr(dense), D, _lib.ptr(sparse), F * D, F, D, B, _lib.ptr(W1), WIDTH, _lib.ptr(b1),
                                                        H, 1, None, 0, _lib.ptr(y1), H, _lib.ptr(pf), st), "fwd")
        _lib.check(L.tzr_dot_interaction_top_bwd_packed(_lib.ptr(dense), D, _lib.ptr(sparse), F * D, F, D, B, _lib.ptr(g1), H, H, _lib.ptr(W1),
                                                        WIDTH, _lib.ptr(scale), _lib.ptr(gd), D, _lib.ptr(gs), F * D, _lib.ptr(pb), st), "bwd")
        out[name] = (y1, gd, gs)
    for a, b, what in zip(out["plain"], out["packed"], ("y1", "gdense", "gsparse")):
        assert not torch.isnan(a).any(), what
        assert torch.equal(a, b), what


def test_pack_holds_every_element_once(dev):
    """the layout is a permutation of W1 plus the 64 zero slots of the pad column, in both copies"""
    from torcheasyrec_amd.dense import pack_w1

    W1 = (torch.arange(H * WIDTH, dtype=torch.float32) + 1).reshape(H, WIDTH).to(dev)
    for p in pack_w1(W1):
        assert p.numel() == H * WIDTH + 64
        assert torch.equal(p.sort().values[64:], W1.flatten()) and int((p == 0).sum()) == 64


def test_optimizer_writes_the_packed_copies(dev):
    from torcheasyrec_amd.dense import FusedDenseAdam, _packed_entry, pack_w1

    torch.manual_seed(1)
    W1 = torch.nn.Parameter(torch.randn(H, WIDTH, device=dev) * 0.05)
    other = torch.nn.Parameter(torch.randn(H, device=dev))
    opt = FusedDenseAdam([other, W1], lr=1e-2)
    before = W1.detach().clone()
    W1.grad, other.grad = torch.randn(H, WIDTH, device=dev), torch.randn(H, device=dev)
    opt.step()
    e = _packed_entry(W1)
    assert e is not None and e.version == W1._version
    assert not torch.equal(W1.detach(), before)
    fwd_p, bwd_p = pack_w1(W1)
    assert torch.equal(e.fwd, fwd_p) and torch.equal(e.bwd, bwd_p)


def test_stale_copies_are_packed_again(dev):
    """W1 overwritten with copy_ behind the optimizer: the next eager forward / backward equals the plain path's"""
    from torcheasyrec_amd.dense import FusedDenseAdam, _packed_entry, interaction_top_loss

    torch.manual_seed(2)
    B = 37
    mk = lambda: (torch.nn.Linear(WIDTH, H).to(dev), torch.nn.Linear(H, 32).to(dev), torch.nn.Linear(32, 1).to(dev))  # noqa: E731
    l1, l2, lo = mk()
    dense = torch.randn(B, D, device=dev, requires_grad=True)
    sparse = torch.randn(B, F * D, device=dev, requires_grad=True)
    y = (torch.rand(B, device=dev) < 0.3).long()
    opt = FusedDenseAdam([p for l in (l1, l2, lo) for p in l.parameters()], lr=1e-2)
    loss, _ = interaction_top_loss(dense, sparse, D, l1, l2, lo, y)
    loss.backward()
    opt.step()
    e = _packed_entry(l1.weight)
    assert e is not None and e.version == l1.weight._version  # in use, and kept up to date by the step
    with torch.no_grad():
        l1.weight.copy_(torch.randn(H, WIDTH, device=dev) * 0.05)
    assert e.version != l1.weight._version
    dense.grad = sparse.grad = None
    loss, logits = interaction_top_loss(dense, sparse, D, l1, l2, lo, y)
    loss.backward()
    assert e.version == l1.weight._version
    # the plain path: the same weights in parameters no optimizer has registered
    m1, m2, mo = mk()
    with torch.no_grad():
        for a, b in zip((l1, l2, lo), (m1, m2, mo)):
            b.weight.copy_(a.weight)
            b.bias.copy_(a.bias)
    assert _packed_entry(m1.weight) is None
    d2, s2 = dense.detach().clone().requires_grad_(True), sparse.detach().clone().requires_grad_(True)
    loss2, logits2 = interaction_top_loss(d2, s2, D, m1, m2, mo, y)
    loss2.backward()
    assert torch.equal(logits, logits2) and torch.equal(loss, loss2)
    assert torch.equal(dense.grad, d2.grad) and torch.equal(sparse.grad, s2.grad)
