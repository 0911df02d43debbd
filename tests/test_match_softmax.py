"""match.match_softmax (tzr_match_softmax_fwd / _bwd, csrc/match_softmax.hip): the match models' similarity head -- normalize,
similarity, temperature, softmax cross entropy and the rank of the positive -- without the score matrix, against the literal
form evaluated in float64 on the CPU (tests/match_softmax_ref.py).  Per kind (loss, lse, dU, dV, sim): max |got - fp64| /
max(1, |fp64|) at or below 4 x the distance of torch's own fp32 literal form to the float64 result on the same inputs, floor
2^-20; no element is left out.  `rank` equals the float64 rank exactly: the inputs are settled (no other column's float64 score
within 2^-14 of its row's positive).

No pass caps its grid (one workgroup per block of 32 own rows) and a wave's tile loop is covered by every case with more than
8 x 16 = 128 rows on the other side (`test_a_wave_walks_more_than_one_tile`), so there is no further loop that runs twice."""
import pytest
import torch

import match_softmax_ref as ref
from torcheasyrec_amd import _lib

MODES = {"sampled": ref.SAMPLED, "in_batch": ref.IN_BATCH}
SETTINGS = {"cosine_T0.05": (True, 0.05), "inner_T1": (False, 1.0)}


def put(x, dev, strided=False):
    """a leaf on `dev`; strided: the column slice [:, 4 : 4 + D] of a buffer 12 wider"""
    if strided:
        buf = torch.zeros(x.shape[0], x.shape[1] + 12)
        buf[:, 4:4 + x.shape[1]] = x
        return buf.to(dev)[:, 4:4 + x.shape[1]].requires_grad_(True)
    return x.to(dev).clone().requires_grad_(True)


def run(u, v, w, mode, cosine, T, want_sim=True):
    from torcheasyrec_amd import match

    assert match.FUSED_MATCH_SOFTMAX and match.match_softmax_ok(u, v, mode, w)
    calls = []
    L = _lib.lib()
    orig = L.tzr_match_softmax_fwd
    L.tzr_match_softmax_fwd = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        loss, rank, sim = match.match_softmax(u, v, mode, cosine, T, w, want_sim=want_sim)
    finally:
        L.tzr_match_softmax_fwd = orig
    assert calls == [1]  # (the kernel, not the literal form)
    du, dv = torch.autograd.grad(loss, [u, v])
    out = {"loss": [loss.detach()], "dU": [du], "dV": [dv], "rank": rank}
    if want_sim:
        out["sim"] = [sim.detach()]
    return out


def kernel_lse(u, v, w, mode, cosine, T):
    """the forward's saved log-sum-exp, through the C entry point's own output"""
    from torcheasyrec_amd.match import _MatchSoftmaxFn

    class Ctx:
        def save_for_backward(self, *ts):
            self.saved = ts

        def mark_non_differentiable(self, *ts):
            pass

    ctx = Ctx()
    _MatchSoftmaxFn.forward(ctx, u.detach(), v.detach(), w, mode, cosine, T, False)
    return ctx.saved[3][0]  # (the saved rows: lse, row maximum, log sum, positive score)


def check_case(dev, mode, B, N, D, cosine, T, weights=None, seed=0, strided=False):
    u, v, w = ref.draw(B, N, D, mode, cosine, T, seed, weights)
    want = ref.literal(u, v, mode, cosine, T, w, torch.float64)
    gaps = ref.gaps(u, v, mode, cosine, T, w, want)
    du, dv, dw = put(u, dev, strided), put(v, dev, strided), None if w is None else w.to(dev)
    got = run(du, dv, dw, mode, cosine, T)
    got["lse"] = [kernel_lse(du, dv, dw, mode, cosine, T)]
    what = f"mode{mode} B{B} N{N} D{D} cosine={cosine} T{T} weights={weights} strided={strided} on {dev.type}"
    ref.check(got, want, gaps, what, ref.KINDS)
    assert got["rank"].dtype == torch.int32 and torch.equal(got["rank"].cpu(), want["rank"]), f"{what}: rank"
    return got, want


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("B", [1, 3, 15, 16, 17, 33])
def test_every_row_tail(dev, B, mode, setting, weights):
    """less than a 16-row tile, exactly one, one row more, a full block of 32 and a row"""
    check_case(dev, MODES[mode], B, 17, 8, *SETTINGS[setting], weights=weights, seed=B)


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("N", [0, 1, 15, 16, 17, 40])
def test_every_negative_count(dev, N, mode, setting, weights):
    """no negative at all (loss 0, gradients 0; the column pass is not launched), one, a tile less one, a tile, a tile and
    one, more than a block (the column pass has two workgroups).  IN_BATCH mode has no N: the same B = 17 each time."""
    got, _ = check_case(dev, MODES[mode], 17, N, 8, *SETTINGS[setting], weights=weights, seed=100 + N)
    if N == 0 and mode == "sampled":
        assert float(got["loss"][0]) == 0.0 and float(got["dU"][0].abs().max()) == 0.0 and float(got["dV"][0].abs().max()) == 0.0


@pytest.mark.parametrize("weights", [None, "rand"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("D", [4, 8, 64, 68, 256])
def test_every_width(dev, D, mode, setting, weights):
    """one float4 a row, less than a 16-column step, the 64-column chunk and the gradient's D <= 64 class exactly, one float4
    past both (the second chunk, the D <= 256 class with a ragged 16-column block), the limit"""
    check_case(dev, MODES[mode], 17, 17, D, *SETTINGS[setting], weights=weights, seed=200 + D)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_wave_walks_more_than_one_tile(dev, mode):
    """The other side is walked in tiles of 16 rows, tile k on wave k mod 8: with 150 negatives (SAMPLED: 10 tiles in the
    forward and the row pass) and B = 150 (10 tiles in the column pass, and in every pass IN_BATCH) waves 0 and 1 run their tile
    loop twice, the second tile of wave 1 a partial one (6 rows).  D = 4: seconds on the emulator."""
    check_case(dev, MODES[mode], 150, 150, 4, True, 0.05, weights="rand", seed=7)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_inputs_and_scores_as_column_slices_of_wider_buffers(dev, mode, setting):
    check_case(dev, MODES[mode], 18, 21, 12, *SETTINGS[setting], weights="rand", seed=11, strided=True)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_scores_into_a_column_slice(dev, mode):
    """`sim` with a row stride above its width, through the C entry point"""
    import ctypes as C

    mode_, cosine, T = MODES[mode], True, 0.05
    u, v, _ = ref.draw(9, 5, 8, mode_, cosine, T, seed=12)
    want = ref.literal(u, v, mode_, cosine, T, None, torch.float64)
    gaps = ref.gaps(u, v, mode_, cosine, T, None, want)
    B, M, Cc = 9, v.shape[0], want["sim"][0].shape[1]
    du, dv = u.to(dev), v.to(dev)
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    loss, lse, rmax, lsum, pos, scale, wide = f(1), f(B), f(B), f(B), f(B), f(1), f(B, Cc + 7)
    ru, rv = f(B).double(), f(M).double()
    rank = torch.zeros(B, dtype=torch.int32, device=dev)
    m = _lib.TzrMatchSoftmax()
    m.B, m.M, m.D, m.mode, m.cosine, m.inv_temperature = B, M, 8, mode_, 1, 1.0 / T
    m.u, m.u_stride, m.v, m.v_stride = du.data_ptr(), 8, dv.data_ptr(), 8
    m.loss, m.lse, m.rmax, m.lsum, m.pos, m.rank, m.scale, m.ru, m.rv = (t.data_ptr() for t in (loss, lse, rmax, lsum, pos, rank, scale, ru, rv))
    m.sim, m.sim_stride = wide[:, 3:].data_ptr(), wide.stride(0)
    L = _lib.lib()
    ws = _lib.workspace(L.tzr_match_softmax_workspace(C.byref(m)), dev)
    m.ws, m.ws_bytes = ws.data_ptr(), ws.numel()
    assert L.tzr_match_softmax_fwd(C.byref(m), _lib.stream_ptr(dev)) == 0
    ref.check({"sim": [wide[:, 3:3 + Cc]], "loss": [loss[0]], "lse": [lse]}, want, gaps, f"strided sim {mode} on {dev.type}", ("sim", "loss", "lse"))
    assert bool(torch.isnan(wide[:, :3]).all()) and bool(torch.isnan(wide[:, 3 + Cc:]).all())  # (nothing outside the slice)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_all_weights_zero(dev, mode, setting):
    """div_no_nan: loss 0, gradients 0, nothing non-finite"""
    cosine, T = SETTINGS[setting]
    u, v, w = ref.draw(17, 17, 8, MODES[mode], cosine, T, seed=13, weights="zero")
    got = run(put(u, dev), put(v, dev), w.to(dev), MODES[mode], cosine, T)
    assert float(got["loss"][0]) == 0.0
    for k in ("dU", "dV"):
        assert bool(torch.isfinite(got[k][0]).all()) and float(got[k][0].abs().max()) == 0.0
    assert bool(torch.isfinite(got["sim"][0]).all())


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_want_sim_changes_nothing_and_two_runs_are_bit_equal(dev, mode, setting):
    cosine, T = SETTINGS[setting]
    u, v, w = ref.draw(33, 40, 8, MODES[mode], cosine, T, seed=14, weights="rand")
    du, dv, dw = put(u, dev), put(v, dev), w.to(dev)
    a = run(du, dv, dw, MODES[mode], cosine, T, want_sim=True)
    b = run(du, dv, dw, MODES[mode], cosine, T, want_sim=False)
    c = run(du, dv, dw, MODES[mode], cosine, T, want_sim=True)
    assert "sim" not in b
    for k in ("loss", "dU", "dV"):
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][0], c[k][0]), k
    assert torch.equal(a["rank"], b["rank"]) and torch.equal(a["rank"], c["rank"]) and torch.equal(a["sim"][0], c["sim"][0])


def test_an_upstream_gradient_scales_both_gradients(dev):
    """the backward reads dL/dloss from device memory"""
    u, v, _ = ref.draw(9, 12, 8, ref.SAMPLED, True, 0.05, seed=15)
    from torcheasyrec_amd import match

    du, dv = put(u, dev), put(v, dev)
    loss, _, _ = match.match_softmax(du, dv, ref.SAMPLED, True, 0.05)
    g1 = torch.autograd.grad(loss, [du, dv], retain_graph=True)
    g2 = torch.autograd.grad(loss * 0.25, [du, dv])
    for a, b in zip(g1, g2):
        assert torch.allclose(a * 0.25, b, rtol=1e-6, atol=1e-9)


def test_outside_the_limits_the_literal_form_runs(dev):
    from torcheasyrec_amd import match

    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    ok = match.match_softmax_ok
    assert ok(z(5, 8), z(9, 8), ref.SAMPLED) and ok(z(5, 8), z(5, 8), ref.SAMPLED) and ok(z(5, 256), z(5, 256), ref.IN_BATCH)
    assert not ok(z(5, 6), z(9, 6), ref.SAMPLED) and not ok(z(5, 260), z(9, 260), ref.SAMPLED) and not ok(z(5, 2), z(9, 2), ref.SAMPLED)
    assert not ok(z(5, 8), z(4, 8), ref.SAMPLED) and not ok(z(5, 8), z(9, 8), ref.IN_BATCH) and not ok(z(0, 8), z(0, 8), ref.IN_BATCH)
    assert not ok(z(5, 8).double(), z(9, 8).double(), ref.SAMPLED) and not ok(z(5, 11)[:, :8], z(9, 8), ref.SAMPLED)
    assert not ok(z(5, 8), z(9, 8), ref.SAMPLED, z(4)) and ok(z(5, 8), z(9, 8), ref.SAMPLED, z(5))
    assert _lib.MATCH_SOFTMAX_MAX_D == 256
    # D = 6: the literal form, the same numbers
    u, v, _ = ref.draw(7, 5, 6, ref.SAMPLED, True, 0.05, seed=16)
    want = ref.literal(u, v, ref.SAMPLED, True, 0.05, None, torch.float64)
    loss, rank, sim = match.match_softmax(put(u, dev), put(v, dev), ref.SAMPLED, True, 0.05, want_sim=True)
    assert abs(float(loss) - float(want["loss"][0])) < 1e-5 and torch.equal(rank.cpu(), want["rank"]) and sim.shape == (7, 6)


def test_fused_off_runs_the_literal_form(dev, monkeypatch):
    from torcheasyrec_amd import match

    monkeypatch.setattr(match, "FUSED_MATCH_SOFTMAX", False)
    for mode in (ref.SAMPLED, ref.IN_BATCH):
        u, v, w = ref.draw(9, 12, 8, mode, True, 0.05, seed=17, weights="rand")
        want = ref.literal(u, v, mode, True, 0.05, w, torch.float64)
        gaps = ref.gaps(u, v, mode, True, 0.05, w, want)
        du, dv = put(u, dev), put(v, dev)
        loss, rank, sim = match.match_softmax(du, dv, mode, True, 0.05, w.to(dev), want_sim=True)
        gu, gv = torch.autograd.grad(loss, [du, dv])
        ref.check({"loss": [loss.detach()], "dU": [gu], "dV": [gv], "sim": [sim.detach()]}, want, gaps, f"literal mode{mode}", ("loss", "dU", "dV", "sim"))
        assert torch.equal(rank.cpu(), want["rank"])
