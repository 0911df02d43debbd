"""The bottom MLP's forward and the weight gradient of W1 as phases of the interaction launches (csrc/interaction_phases.hip): the
same device bodies on the same tiles per workgroup, so every output is BIT-identical to the two launches each entry stands for --
at batch sizes around the tile (16) and slice (32) sizes, with more tiles than workgroups, with workgroups that have no tile in
one phase but work in the other, and with the step's switches each way."""
import ctypes as C

import pytest
import torch

from torcheasyrec_amd import _lib, dense
from torcheasyrec_amd.criteo import NUM_DENSE, SPARSE_KEYS, criteo_tables, synthetic_batch
from torcheasyrec_amd.dense import FusedDenseAdam, pack_w1
from torcheasyrec_amd.dlrm import DLRM
from torcheasyrec_amd.embedding import SparseOptimizerConfig

D, F, H = 16, 26, 64
WIDTH = 27 * 26 // 2 + 27 * D
H1, H2 = 64, 16  # the bottom MLP: K0 -> 64 -> 16


def _rand(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g).to(dev)


def _forward_pair(dev, B, K0):
    """(ha, hb, y1) of tzr_mlp2_fwd + tzr_dot_interaction_top_fwd_packed, and of the one launch"""
    L = _lib.lib()
    r = _rand(dev, 100 * B + K0)
    x, Wa, ba, Wb, bb = r(B, K0), r(H1, K0) * 0.3, r(H1) * 0.1, r(H2, H1) * 0.2, r(H2) * 0.1
    sparse, W1, b1 = r(B, F * D), r(H, WIDTH) * 0.05, r(H)
    fwd_p, _ = pack_w1(W1)
    st = _lib.stream_ptr(dev)
    out = []
    for one in (False, True):
        ha, hb, y1 = (torch.full(s, float("nan"), device=dev) for s in ((B, H1), (B, H2), (B, H)))
        mlp2 = (_lib.ptr(x), K0, B, K0, _lib.ptr(Wa), _lib.ptr(ba), H1, _lib.ptr(Wb), _lib.ptr(bb), H2, _lib.ptr(ha), H1, _lib.ptr(hb), H2)
        head = (_lib.ptr(hb), H2, _lib.ptr(sparse), F * D, F, D)
        tail = (_lib.ptr(W1), WIDTH, _lib.ptr(b1), H, 1, None, 0, _lib.ptr(y1), H, _lib.ptr(fwd_p))
        if one:
            _lib.check(L.tzr_dot_interaction_top_fwd_mlp2(*mlp2, *head, *tail, st), "fwd_mlp2")
        else:
            _lib.check(L.tzr_mlp2_fwd(*mlp2, st), "mlp2_fwd")
            _lib.check(L.tzr_dot_interaction_top_fwd_packed(*head, B, *tail, st), "fwd_packed")
        out.append((ha, hb, y1))
    return out


def _assert_same(two, one, names):
    for a, b, what in zip(two, one, names):
        assert not torch.isnan(a).any() and not torch.isnan(b).any(), what
        assert torch.equal(a, b), what


# one sample; a tile less one, a tile, a tile and one; sixteen tiles less one sample (every wave of ONE workgroup would have a
# tile, but the grid gives every tile its own workgroup: fifteen waves idle in phase 0); 38 tiles; more tiles than workgroups
@pytest.mark.parametrize("K0", [13, 16])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 255, 600, 4099])
def test_forward_with_the_bottom_mlp_as_phase_0_is_bit_identical(dev, B, K0):
    two, one = _forward_pair(dev, B, K0)
    _assert_same(two, one, ("ha", "hb", "y1"))


# 38 tiles on 2 workgroups: a wave takes more than one tile in phase 0 (waves 0 .. 2 of either workgroup two) and some none; 2
# tiles on 3 workgroups asked for: the grid is the tiles
@pytest.mark.parametrize("B,wgs", [(600, 2), (17, 3)])
def test_forward_phase_0_on_few_workgroups(dev, B, wgs):
    assert _lib.lib().tzr_tune(b"it_wgs", wgs) == 0
    two, one = _forward_pair(dev, B, 13)
    _assert_same(two, one, ("ha", "hb", "y1"))


def test_forward_refuses_other_shapes(dev):
    """z wanted, no packed W1, another dense vector than hb, a bottom MLP the MFMA body does not take: TZR_ERR_UNSUPPORTED"""
    L = _lib.lib()
    B, K0 = 16, 13
    r = _rand(dev, 7)
    x, Wa, ba, Wb, bb = r(B, K0), r(H1, K0), r(H1), r(H2, H1), r(H2)
    sparse, W1, b1 = r(B, F * D), r(H, WIDTH), r(H)
    fwd_p, _ = pack_w1(W1)
    ha, hb, y1, z, other = r(B, H1), r(B, H2), r(B, H), r(B, WIDTH), r(B, H2)
    st = _lib.stream_ptr(dev)

    def call(K0=K0, dense_=hb, z_=None, pk=fwd_p):
        return L.tzr_dot_interaction_top_fwd_mlp2(_lib.ptr(x), 13, B, K0, _lib.ptr(Wa), _lib.ptr(ba), H1, _lib.ptr(Wb), _lib.ptr(bb), H2,
                                                  _lib.ptr(ha), H1, _lib.ptr(hb), H2, _lib.ptr(dense_), H2, _lib.ptr(sparse), F * D, F, D,
                                                  _lib.ptr(W1), WIDTH, _lib.ptr(b1), H, 1, _lib.ptr(z_), WIDTH, _lib.ptr(y1), H, _lib.ptr(pk), st)

    assert call() == _lib.TZR_OK
    assert call(z_=z) == _lib.TZR_ERR_UNSUPPORTED
    assert call(pk=None) == _lib.TZR_ERR_UNSUPPORTED
    assert call(dense_=other) == _lib.TZR_ERR_UNSUPPORTED
    assert L.tzr_tune(b"mlp_mfma", -1) == 0
    assert call() == _lib.TZR_ERR_UNSUPPORTED


def _reduced(dev, blob):
    """dW1 out of the slices by the existing reduce path: the dense optimizer's launch, as `materialize_pending` runs it"""
    dW = torch.full((H, WIDTH), float("nan"), device=dev)
    dense._defer(dW, "wgrad", (), blob, ())
    dense.materialize_pending([dW])
    return dW


# one sample; a tile and one; 3 backward workgroups against 32 of the weight gradient; 38 against 32; 256 against 160
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("B", [1, 17, 48, 600, 5000])
def test_backward_with_the_weight_gradient_as_phase_2_is_bit_identical(dev, B, scaled):
    L = _lib.lib()
    r = _rand(dev, B)
    hb, sparse, W1, g1 = r(B, D), r(B, F * D), r(H, WIDTH) * 0.05, r(B, H)
    scale = torch.full((1,), 0.37, device=dev) if scaled else None
    _, bwd_p = pack_w1(W1)
    st = _lib.stream_ptr(dev)
    nbytes = L.tzr_dot_interaction_top_wgrad_workspace(F, D, 1, H)
    out = []
    for one in (False, True):
        gd, gs = torch.full_like(hb, float("nan")), torch.full_like(sparse, float("nan"))
        ws = torch.full((nbytes // 4,), float("nan"), device=dev)
        blob = _lib.TzrWgradParts()
        bwd = (_lib.ptr(hb), D, _lib.ptr(sparse), F * D, F, D, B, _lib.ptr(g1), H, H, _lib.ptr(W1), WIDTH, _lib.ptr(scale), _lib.ptr(gd), D,
               _lib.ptr(gs), F * D, _lib.ptr(bwd_p))
        if one:
            _lib.check(L.tzr_dot_interaction_top_bwd_wgrad_parts(*bwd, _lib.ptr(ws), nbytes, C.byref(blob), st), "bwd_wgrad_parts")
        else:
            _lib.check(L.tzr_dot_interaction_top_bwd_packed(*bwd, st), "bwd_packed")
            _lib.check(L.tzr_dot_interaction_top_wgrad_parts(_lib.ptr(hb), D, _lib.ptr(sparse), F * D, F, D, B, _lib.ptr(g1), H, H, _lib.ptr(scale),
                                                             _lib.ptr(ws), nbytes, C.byref(blob), st), "wgrad_parts")
        out.append((gd, gs, _reduced(dev, blob), ws))
    _assert_same(out[0][:3], out[1][:3], ("gd", "gs", "dW1"))


@pytest.fixture
def _plain_flag():
    dense.FUSE_FINISH = False
    dense._PENDING.clear()
    yield
    dense.FUSE_FINISH = False
    dense._PENDING.clear()


def _step(dev, monkeypatch, fwd_phase, wgrad_phase):
    """one DLRM-Criteo training step, B = 96, tables capped: (loss, logits, every dense parameter after the step, launches)"""
    monkeypatch.setattr(dense, "PHASE_MLP2_FWD", fwd_phase)
    monkeypatch.setattr(dense, "PHASE_WGRAD", wgrad_phase)
    torch.manual_seed(0)
    rows = [300] * 26
    model = DLRM(criteo_tables(rows, init="seeded"), SPARSE_KEYS, NUM_DENSE, device=dev, sparse_optimizer=SparseOptimizerConfig(kind="sgd", lr=0.01))
    params = list(model.dense_parameters())
    dense.FUSE_FINISH = False
    opt = FusedDenseAdam(params, lr=1e-2, weight_decay=1e-3, fuse_finish=True)
    before = list(dense.PHASE_LAUNCHES)
    d, kjt, y = synthetic_batch(0, 96, rows)
    loss, logits = model.forward_loss(d.to(dev), kjt.to(dev), y.to(dev))
    with dense.root_loss():
        loss.backward(gradient=dense.unit_gradient(loss))
    opt.step()
    assert not dense._PENDING
    launches = [a - b for a, b in zip(dense.PHASE_LAUNCHES, before)]
    return loss.detach().cpu(), logits.detach().cpu(), [p.detach().cpu().clone() for p in params], launches


def test_training_step_is_bit_identical_with_each_switch(dev, monkeypatch, _plain_flag):
    ref = _step(dev, monkeypatch, False, False)
    assert ref[3] == [0, 0]
    for fwd_phase, wgrad_phase in ((True, False), (False, True), (True, True)):
        got = _step(dev, monkeypatch, fwd_phase, wgrad_phase)
        assert got[3] == [int(fwd_phase), int(wgrad_phase)], "the one-launch entries were taken"
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
        for a, b in zip(ref[2], got[2]):
            assert torch.equal(a, b)
