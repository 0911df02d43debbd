"""tzr_mlp2_fwd, tzr_mlp2_bwd / tzr_mlp2_bwd_parts and tzr_mlp_tail (csrc/mlp_ops.hip: the general LDS-tiled VALU kernels;
csrc/mlp_mfma.hip + csrc/mlp2_fwd16_body.h: the MFMA kernels of the DLRM-Criteo shapes) called directly through the C ABI, every
row-strided operand a column slice of a wider NaN-filled buffer, against the float64 restatement of tests/mlp_ref.py.

Bound, per tensor kind (forward: ha, hb; backward: dWb, dbb, dWa, dba; tail: logits, loss, g1, db1, dW2, db2, dw3, db3):
|ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the distance of torch's literal fp32 form on the CPU to float64 on
the same inputs (the rule of tests/test_ln_mask_kernel.py).  Every case runs twice and must give the same bits; nothing outside
the slices may be written, and every element inside them must be (the outputs start out NaN-filled; a NaN fails the bound).

Measured over the cases below, the kernels' distance over the literal form's (printed per case and kind as `ours / literal`).
On the lane emulator: ha 0.65 - 2.65, hb 0.56 - 6.84, dWb 0.18 - 2.68, dbb 0.10 - 5.73, dWa 0.38 - 1.87, dba 0.16 - 2.12; logits
0.54 - 71.22, loss 0.01 - 36.02, g1 0.46 - 2.48, db1 0.32 - 4.07, dW2 0.25 - 2.29, db2 0.25 - 3.19, dw3 0.52 - 3.65, db3 0.00 - 37.07;
the largest, logits 71.22, at the tail (B 1, 63, 32).  On the device: ha 0.65 - 2.93, hb 0.42 - 6.84, dWb 0.30 - 2.42, dbb 0.10 - 5.73,
dWa 0.21 - 11.64, dba 0.16 - 2.02; logits 0.49 - 71.22, loss 0.01 - 36.02, g1 0.46 - 2.48, db1 0.32 - 2.10, dW2 0.08 - 1.61, db2
0.18 - 3.19, dw3 0.44 - 3.90, db3 0.00 - 51.42; the largest again logits 71.22 at (B 1, 63, 32), then db3 51.42 at the tail (B 130, 8, 4).
Seven kinds pass 4 on one backend or the other (hb, dbb, dWa, logits, loss, db1, db3): every such case is one whose error lies UNDER the floor
-- the largest error among them is 6.8e-7 on the emulator (dbb, B 65, (5, 64, 16)) and 7.5e-7 on the device (dWa, B 130, (1, 1, 1)),
against 2^-20 = 9.5e-7 -- and it is the denominator that is small there, not the kernel that is far: with one sample or one unit the
literal form is a single short dot product that lands within 1e-9 of float64 by chance (logits at B 1: gap 4e-10, ours 3e-8, half
an ulp of the logit).  The sums that pass 4 are the kernels' chains: db3 and the loss are added by one thread, 64 terms of a tile
after another (`v += sdl[r]`), on expf / log1pf in fp32, where torch sums pairwise; dbb on the matrix cores is a running sum per
lane over the wave's tiles, then a shuffle tree, the four waves in order, then the finish.  Among the figures ABOVE the floor (56 on
the emulator, 57 on the device) the largest ratio is 2.68 (dWb at B 130, (5, 33, 7); on the device dbb 2.68 at B 193, (13, 64, 16)):
where the factor 4 carries the bound it suffices, with room.
"""
import ctypes as C

import pytest
import torch

import mlp_ref as ref
from torcheasyrec_amd import _lib

# the constants of csrc/mlp_ops.hip and csrc/mlp_mfma.hip the shapes below are chosen against
ML_TS, ML_MAX_WG, ML_FWD_WG = 64, 512, 1024  # VALU: samples per tile; workgroups of backward and tail; of the forward
MM_TS, MM_WAVES, MM_MAX_WG, MM_FWD_WG = 16, 4, 512, 1024  # MFMA: samples per wave and turn; waves per workgroup; the same two caps
ML_MAX = (32, 64, 32)  # K0, H1, H2 the entries take
CRITEO = (13, 64, 16)  # bottom MLP; the tail of the top MLP is (64, 32)
TAIL = (64, 32)

MFMA_K0 = (1, 3, 4, 5, 13, 15, 16)
MFMA_B = (1, 15, 16, 17, 63, 64, 65, 193)
KNOB_B = 133  # knob 1: one workgroup, tiles 9 -> waves take 3, 2, 2, 2 turns, the last tile holds 5 samples; knob 2: two workgroups
VALU_SHAPES = ((1, 1, 1), (3, 8, 4), (5, 33, 7), (32, 64, 32), (17, 64, 16), (13, 63, 16), (13, 64, 15))
VALU_B = (1, 63, 64, 65, 130)
TAIL_VALU_SHAPES = ((1, 1), (8, 4), (24, 9), (33, 7), (64, 31), (63, 32))
CAP_B_BWD = ML_MAX_WG * ML_TS + ML_TS + 5  # 32837: VALU, workgroup 0 takes a second tile, the last tile is partial; MFMA, 2053 tiles on 2048 waves
CAP_B_FWD = ML_FWD_WG * ML_TS + ML_TS + 5  # 65605: the same for the two forwards (4101 tiles on 4096 waves)
CAP_VALU = (3, 8, 4)


# ---- operands as column slices -----------------------------------------------------------------------------------------------
class Slice:
    """a [B, n] tensor as a column slice `v` of a wider NaN-filled buffer `w`:
    "aligned": the row stride a multiple of 4 floats, the slice 16 bytes into a row (what the MFMA kernels require)
    "odd":     the row stride 4 k + 1 floats, the slice at a 16-byte aligned address (`stride & 3` fails alone)
    "shift":   the row stride a multiple of 4 floats, the slice one float into an aligned row (`pointer & 15` fails alone)"""

    def __init__(self, t, dev, how):
        t = t.reshape(t.shape[0], -1)
        B, n = t.shape
        n4 = (n + 3) & ~3
        width, self.start = {"aligned": (n4 + 8, 4), "odd": (n4 + 9, 4), "shift": (n4 + 8, 1)}[how]
        self.w = torch.full((B, width), float("nan"), dtype=torch.float32, device=dev)
        self.n = n
        self.v = self.w[:, self.start:self.start + n]
        self.v.copy_(t)
        assert self.w.data_ptr() % 16 == 0
        a, s = self.v.data_ptr() & 15, self.v.stride(0) & 3
        assert (a, s) == {"aligned": (0, 0), "odd": (0, 1), "shift": (4, 0)}[how], (how, a, s)

    def untouched(self):
        return bool(torch.isnan(self.w[:, :self.start]).all()) and bool(torch.isnan(self.w[:, self.start + self.n:]).all())


def _dev(t, dev, shift=False):
    """a contiguous parameter on the device; `shift`: as a view one float into a flat buffer (4-byte aligned only)"""
    if t is None:
        return None
    if not shift:
        return t.to(dev).contiguous()
    flat = torch.full((t.numel() + 1,), float("nan"), dtype=torch.float32, device=dev)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() & 15 == 4
    return v


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _tune(knob):
    assert _lib.lib().tzr_tune(b"mlp_mfma", knob) == 0


def run_mlp2(dev, x, Wa, ba, Wb, bb, dhb, ha_in, hb_in, knob=0, place="aligned", over=None, wb_shift=False, do=("fwd", "bwd"),
             null_out=(), parts=False):
    """tzr_mlp2_fwd on (x, Wa, ba, Wb, bb) -> ha, hb; tzr_mlp2_bwd on the GIVEN (dhb, hb_in, ha_in, x, Wb) -> dWb, dbb, dWa, dba.
    `place`: how every strided operand lies (x: always "odd", no kernel cares), `over`: operand name -> another placement;
    `null_out`: outputs passed as null; `parts`: tzr_mlp2_bwd_parts instead -> "G", "P", "rows" [G, P]"""
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    over = over or {}
    how = lambda name: over.get(name, place)  # noqa: E731
    B, K0 = x.shape
    H1, H2 = Wa.shape[0], Wb.shape[0]
    Wa_, ba_, bb_ = (_dev(t, dev) for t in (Wa, ba, bb))
    Wb_ = _dev(Wb, dev, shift=wb_shift)
    xs = Slice(x, dev, "odd")
    _tune(knob)
    out = {}
    if "fwd" in do:
        ha, hb = Slice(torch.zeros(B, H1), dev, how("ha")), Slice(torch.zeros(B, H2), dev, how("hb"))
        ha.v.fill_(float("nan"))
        hb.v.fill_(float("nan"))
        assert lib.tzr_mlp2_fwd(p(xs.v), xs.v.stride(0), B, K0, p(Wa_), p(ba_), H1, p(Wb_), p(bb_), H2, p(ha.v), ha.v.stride(0), p(hb.v),
                                hb.v.stride(0), st) == 0
        assert ha.untouched() and hb.untouched()  # nothing outside the slices was written
        out.update(ha=[ha.v], hb=[hb.v])
    if "bwd" in do:
        g, hbi, hai = Slice(dhb, dev, how("dhb")), Slice(hb_in, dev, how("hb")), Slice(ha_in, dev, how("ha"))
        ws = _lib.workspace(lib.tzr_mlp_workspace(), dev)
        args = (p(g.v), g.v.stride(0), p(hbi.v), hbi.v.stride(0), p(hai.v), hai.v.stride(0), p(xs.v), xs.v.stride(0), B, K0, H1, H2, p(Wb_))
        if parts:
            ws.fill_(255)  # (every float of it a NaN: a row element nobody wrote shows)
            G, P = C.c_int(-1), C.c_int(-1)
            assert lib.tzr_mlp2_bwd_parts(*args, p(ws), ws.numel(), C.byref(G), C.byref(P), st) == 0
            out.update(G=G.value, P=P.value, rows=[ws[:G.value * P.value * 4].view(torch.float32).view(G.value, P.value).clone()])
        else:
            o = {"dWa": _nan(dev, H1, K0), "dba": _nan(dev, H1), "dWb": _nan(dev, H2, H1), "dbb": _nan(dev, H2)}
            q = {k: (None if k in null_out else p(t)) for k, t in o.items()}
            assert lib.tzr_mlp2_bwd(*args, q["dWa"], q["dba"], q["dWb"], q["dbb"], p(ws), ws.numel(), st) == 0
            for k in null_out:
                assert bool(torch.isnan(o[k]).all())
            out.update({k: [t] for k, t in o.items() if k not in null_out})
    return out


def run_tail(dev, y1, labels, W2, b2, w3, b3, knob=0, place="aligned", over=None, w2_shift=False):
    """tzr_mlp_tail -> logits, loss, g1, db1, dW2, db2, dw3, db3"""
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    over = over or {}
    B, H1 = y1.shape
    H2 = W2.shape[0]
    b2_, w3_, b3_ = (_dev(t, dev) for t in (b2, w3, b3))
    W2_ = _dev(W2, dev, shift=w2_shift)
    y = labels.to(dev).contiguous()
    ys, g1 = Slice(y1, dev, over.get("y1", place)), Slice(torch.zeros(B, H1), dev, over.get("g1", place))
    g1.v.fill_(float("nan"))
    logits, dW2, db2, dw3, scal, db1 = _nan(dev, B), _nan(dev, H2, H1), _nan(dev, H2), _nan(dev, H2), _nan(dev, 2), _nan(dev, H1)
    ws = _lib.workspace(lib.tzr_mlp_workspace(), dev)
    _tune(knob)
    assert lib.tzr_mlp_tail(p(ys.v), ys.v.stride(0), p(y), y.element_size(), int(y.is_floating_point()), B, H1, p(W2_), p(b2_), H2, p(w3_),
                            p(b3_), p(logits), p(g1.v), g1.v.stride(0), p(dW2), p(db2), p(dw3), p(scal), p(db1), p(ws), ws.numel(), st) == 0
    assert g1.untouched()
    return {"logits": [logits], "loss": [scal[1:2]], "g1": [g1.v], "db1": [db1], "dW2": [dW2], "db2": [db2], "dw3": [dw3], "db3": [scal[0:1]]}


def _bit_equal(a, b, kinds=None):
    """the same bits: the int32 views are compared, so 0.0 and -0.0 differ (and a NaN would equal itself: `_finite` is what
    looks for those)"""
    kinds = [k for k in a if isinstance(a[k], list)] if kinds is None else kinds
    return all(torch.equal(p.contiguous().view(torch.int32), q.contiguous().view(torch.int32)) for k in kinds for p, q in zip(a[k], b[k]))


def _finite(got):
    """no output element was left as the NaN it was filled with, and none was computed as one"""
    return all(bool(torch.isfinite(t).all()) for v in got.values() if isinstance(v, list) for t in v)


def _twice(run):
    """the case run twice: every output written and finite, the same bits both times -> the first run's outputs"""
    a, b = run(), run()
    assert _finite(a) and _finite(b), "an output element is NaN or infinite (unwritten, or computed so)"
    assert sorted(a) == sorted(b) and _bit_equal(a, b) and all(a[k] == b[k] for k in a if not isinstance(a[k], list)), "two runs of the same case differ"
    return a


def _judge(got, want, lit, what, kinds):
    assert _finite(got), f"{what}: an output element is NaN or infinite"
    gaps = {k: ref.rel_err(lit[k], want[k]) for k in kinds}
    for k in kinds:
        if gaps[k] > 0:
            print(f"{what} {k}: ours / literal {ref.rel_err(got[k], want[k]) / gaps[k]:.2f}")
    ref.check(got, want, gaps, what, kinds)
    return gaps


# ---- the cases ---------------------------------------------------------------------------------------------------------------
_REFS = {}


def mlp2_case(B, K0, H1, H2):
    """inputs, the given activations, float64 truth and fp32 literal of one shape: computed once, shared, never written"""
    key = ("mlp2", B, K0, H1, H2)
    if key not in _REFS:
        x, Wa, ba, Wb, bb, dhb = ins = ref.draw_mlp2(B, K0, H1, H2, seed=B * 131 + K0 * 17 + H1 * 3 + H2)
        ha, hb = ref.given_activations(x, Wa, ba, Wb, bb)
        want = dict(ref.mlp2_fwd_literal(x, Wa, ba, Wb, bb), **ref.mlp2_bwd_literal(dhb, hb, ha, x, Wb))
        lit = dict(ref.mlp2_fwd_literal(x, Wa, ba, Wb, bb, dtype=torch.float32), **ref.mlp2_bwd_literal(dhb, hb, ha, x, Wb, dtype=torch.float32))
        _REFS[key] = (ins + (ha, hb), want, lit)
    return _REFS[key]


def tail_case(B, H1, H2, **kw):
    key = ("tail", B, H1, H2, tuple(sorted(kw.items())))
    if key not in _REFS:
        ins = ref.draw_tail(B, H1, H2, seed=B * 137 + H1 * 19 + H2, **kw)
        _REFS[key] = (ins, ref.tail_literal(*ins), ref.tail_literal(*ins, dtype=torch.float32))
    return _REFS[key]


def check_mlp2(dev, B, K0, H1, H2, knob, place, do=("fwd", "bwd")):
    ins, want, lit = mlp2_case(B, K0, H1, H2)
    kinds = (ref.FWD_KINDS if "fwd" in do else ()) + (ref.BWD_KINDS if "bwd" in do else ())
    got = _twice(lambda: run_mlp2(dev, *ins, knob=knob, place=place, do=do))
    _judge(got, want, lit, f"mlp2 (B {B}, {K0}, {H1}, {H2}) knob {knob} on {dev.type}", kinds)
    return got


def check_tail(dev, B, H1, H2, knob, place, **kw):
    ins, want, lit = tail_case(B, H1, H2, **kw)
    got = _twice(lambda: run_tail(dev, *ins, knob=knob, place=place))
    _judge(got, want, lit, f"tail (B {B}, {H1}, {H2}) knob {knob} {kw or ''} on {dev.type}", ref.TAIL_KINDS)
    return got


@pytest.mark.parametrize("B", MFMA_B)
@pytest.mark.parametrize("K0", MFMA_K0)
def test_mlp2_mfma_family(dev, K0, B):
    check_mlp2(dev, B, K0, CRITEO[1], CRITEO[2], 0, "aligned")


@pytest.mark.parametrize("knob", [1, 2])
def test_mlp2_mfma_several_turns_per_wave(dev, knob):
    check_mlp2(dev, KNOB_B, *CRITEO, knob, "aligned")


@pytest.mark.parametrize("B", VALU_B)
@pytest.mark.parametrize("K0,H1,H2,knob", [s + (0,) for s in VALU_SHAPES] + [CRITEO + (-1,)])
def test_mlp2_valu_family(dev, K0, H1, H2, knob, B):
    check_mlp2(dev, B, K0, H1, H2, knob, "odd")


@pytest.mark.parametrize("B", MFMA_B)
def test_tail_mfma_family(dev, B):
    check_tail(dev, B, *TAIL, 0, "aligned")


@pytest.mark.parametrize("knob", [1, 2])
def test_tail_mfma_several_turns_per_wave(dev, knob):
    check_tail(dev, KNOB_B, *TAIL, knob, "aligned")


@pytest.mark.parametrize("B", VALU_B)
@pytest.mark.parametrize("H1,H2,knob", [s + (0,) for s in TAIL_VALU_SHAPES] + [TAIL + (-1,)])
def test_tail_valu_family(dev, H1, H2, knob, B):
    check_tail(dev, B, H1, H2, knob, "odd")


# ---- workgroup caps: a grid-stride loop's second turn, one case per kernel ------------------------------------------------------
def test_cap_mfma_backward(dev):
    check_mlp2(dev, CAP_B_BWD, *CRITEO, 0, "aligned", do=("bwd",))


def test_cap_valu_backward(dev):
    check_mlp2(dev, CAP_B_BWD, *CAP_VALU, 0, "odd", do=("bwd",))


def test_cap_mfma_tail(dev):
    check_tail(dev, CAP_B_BWD, *TAIL, 0, "aligned")


def test_cap_valu_tail(dev):
    check_tail(dev, CAP_B_BWD, *CAP_VALU[1:], 0, "odd")


def test_cap_mfma_forward(dev):
    check_mlp2(dev, CAP_B_FWD, *CRITEO, 0, "aligned", do=("fwd",))


def test_cap_valu_forward(dev):
    check_mlp2(dev, CAP_B_FWD, *CAP_VALU, 0, "odd", do=("fwd",))


# ---- alignment fallbacks: an operand the MFMA kernels cannot take goes to the VALU kernel ----------------------------------------
ALIGN_B = 193
# placement -> (run_mlp2 / run_tail keywords, the kinds whose entry point must have fallen back)
MLP2_FALLBACKS = {
    "rows 4 k + 1 floats wide": (dict(place="odd"), ref.FWD_KINDS + ref.BWD_KINDS),
    "ha one float into a row": (dict(over={"ha": "shift"}), ref.FWD_KINDS + ref.BWD_KINDS),
    "hb one float into a row": (dict(over={"hb": "shift"}), ref.BWD_KINDS),  # (the forward stores hb 4 bytes at a time)
    "dhb one float into a row": (dict(over={"dhb": "shift"}), ref.BWD_KINDS),
    "Wb one float into a flat buffer": (dict(wb_shift=True), ref.FWD_KINDS),  # (the backward reads Wb 4 bytes at a time)
}
TAIL_FALLBACKS = {
    "rows 4 k + 1 floats wide": dict(place="odd"),
    "y1 one float into a row": dict(over={"y1": "shift"}),
    "g1 one float into a row": dict(over={"g1": "shift"}),
    "W2 one float into a flat buffer": dict(w2_shift=True),
}


@pytest.mark.parametrize("where", list(MLP2_FALLBACKS))
def test_mlp2_alignment_fallback(dev, where):
    """within bound, and the same bits as knob -1: both are then the VALU kernel (Slice / _dev assert the alignment bits)"""
    kw, fell = MLP2_FALLBACKS[where]
    ins, want, lit = mlp2_case(ALIGN_B, *CRITEO)
    got = _twice(lambda: run_mlp2(dev, *ins, knob=0, **kw))
    _judge(got, want, lit, f"mlp2 {where} on {dev.type}", ref.FWD_KINDS + ref.BWD_KINDS)
    assert _bit_equal(got, _twice(lambda: run_mlp2(dev, *ins, knob=-1, **kw)), fell), f"{where}: not the general kernel's bits"


@pytest.mark.parametrize("where", list(TAIL_FALLBACKS))
def test_tail_alignment_fallback(dev, where):
    kw = TAIL_FALLBACKS[where]
    ins, want, lit = tail_case(ALIGN_B, *TAIL)
    got = _twice(lambda: run_tail(dev, *ins, knob=0, **kw))
    _judge(got, want, lit, f"tail {where} on {dev.type}", ref.TAIL_KINDS)
    assert _bit_equal(got, _twice(lambda: run_tail(dev, *ins, knob=-1, **kw))), f"{where}: not the general kernel's bits"


def test_aligned_operands_take_the_mfma_kernels(dev):
    """the other side of the fallback tests: on aligned operands knob 0 and knob -1 are two kernels that add in two orders, so
    over 193 samples some bit of every entry point's output differs (were they equal, knob 0 would not have reached mlp_mfma.hip)"""
    ins, _, _ = mlp2_case(ALIGN_B, *CRITEO)
    a, b = _twice(lambda: run_mlp2(dev, *ins, knob=0)), _twice(lambda: run_mlp2(dev, *ins, knob=-1))
    assert not _bit_equal(a, b, ref.FWD_KINDS) and not _bit_equal(a, b, ref.BWD_KINDS)
    ins, _, _ = tail_case(ALIGN_B, *TAIL)
    assert not _bit_equal(_twice(lambda: run_tail(dev, *ins, knob=0)), _twice(lambda: run_tail(dev, *ins, knob=-1)))


# ---- optional arguments and label types --------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["mfma", "valu"])
@pytest.mark.parametrize("null", [("ba",), ("bb",), ("ba", "bb")])
def test_mlp2_null_biases(dev, family, null):
    B = 65
    K0, H1, H2 = CRITEO if family == "mfma" else (5, 33, 7)
    x, Wa, ba, Wb, bb, dhb = ref.draw_mlp2(B, K0, H1, H2, seed=7 + len(null))
    ba, bb = (None if "ba" in null else ba), (None if "bb" in null else bb)
    got = _twice(lambda: run_mlp2(dev, x, Wa, ba, Wb, bb, dhb, None, None, place="aligned" if family == "mfma" else "odd", do=("fwd",)))
    _judge(got, ref.mlp2_fwd_literal(x, Wa, ba, Wb, bb), ref.mlp2_fwd_literal(x, Wa, ba, Wb, bb, dtype=torch.float32),
           f"mlp2 {family} without {null} on {dev.type}", ref.FWD_KINDS)


@pytest.mark.parametrize("family", ["mfma", "valu"])
@pytest.mark.parametrize("null", [("b2",), ("b3",), ("b2", "b3")])
def test_tail_null_biases(dev, family, null):
    B = 65
    H1, H2 = TAIL if family == "mfma" else (33, 7)
    y1, labels, W2, b2, w3, b3 = ref.draw_tail(B, H1, H2, seed=11 + len(null), bias2="b2" not in null)
    b2, b3 = (None if "b2" in null else b2), (None if "b3" in null else b3)
    got = _twice(lambda: run_tail(dev, y1, labels, W2, b2, w3, b3, place="aligned" if family == "mfma" else "odd"))
    _judge(got, ref.tail_literal(y1, labels, W2, b2, w3, b3), ref.tail_literal(y1, labels, W2, b2, w3, b3, dtype=torch.float32),
           f"tail {family} without {null} on {dev.type}", ref.TAIL_KINDS)


@pytest.mark.parametrize("family", ["mfma", "valu"])
def test_mlp2_bwd_null_bias_gradients(dev, family):
    """null d_dba / d_dbb: the other outputs keep their bits"""
    K0, H1, H2 = CRITEO if family == "mfma" else (5, 33, 7)
    place = "aligned" if family == "mfma" else "odd"
    ins, _, _ = mlp2_case(65, K0, H1, H2)
    full = _twice(lambda: run_mlp2(dev, *ins, place=place, do=("bwd",)))
    for null in (("dba",), ("dbb",), ("dba", "dbb")):
        got = _twice(lambda: run_mlp2(dev, *ins, place=place, do=("bwd",), null_out=null))
        assert sorted(got) == sorted(k for k in ref.BWD_KINDS if k not in null)
        assert _bit_equal(got, full, list(got))


@pytest.mark.parametrize("family", ["mfma", "valu"])
@pytest.mark.parametrize("labels", ref.LABEL_KINDS)
def test_tail_label_types(dev, family, labels):
    H1, H2 = TAIL if family == "mfma" else (24, 9)
    got = check_tail(dev, 65, H1, H2, 0, "aligned" if family == "mfma" else "odd", labels=labels)
    if labels != "soft":  # the three {0, 1} encodings are one case (the same seed draws the same inputs): the same bits
        ins, _, _ = tail_case(65, H1, H2, labels="int64")
        assert _bit_equal(got, _twice(lambda: run_tail(dev, *ins, place="aligned" if family == "mfma" else "odd")))


# ---- masks and range ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["mfma", "valu"])
def test_mlp2_bwd_masks_on_exact_zeros(dev, family):
    """ha / hb with exact 0.0 and -0.0, one dead unit each (an all-zero column: its gradients are exactly 0.0) and one all-zero row"""
    B = 70
    K0, H1, H2 = CRITEO if family == "mfma" else (5, 33, 7)
    x, Wa, ba, Wb, bb, dhb = ref.draw_mlp2(B, K0, H1, H2, seed=23)
    g = torch.Generator().manual_seed(29)
    ha, hb = torch.relu(torch.randn(B, H1, generator=g)), torch.relu(torch.randn(B, H2, generator=g))
    da, db = H1 // 2, H2 // 2
    ha[:, da], hb[:, db], ha[3], hb[5] = 0.0, 0.0, 0.0, 0.0
    assert ref.negative_zeros(ha, every=3) > B and ref.negative_zeros(hb, every=3) > B // 2
    assert bool(torch.signbit(ha[:, da]).any()) and bool(torch.signbit(hb[:, db]).any()) and bool((ha[:, da] == 0).all())
    want, lit = ref.mlp2_bwd_literal(dhb, hb, ha, x, Wb), ref.mlp2_bwd_literal(dhb, hb, ha, x, Wb, dtype=torch.float32)
    got = _twice(lambda: run_mlp2(dev, x, Wa, ba, Wb, bb, dhb, ha, hb, place="aligned" if family == "mfma" else "odd", do=("bwd",)))
    _judge(got, want, lit, f"mlp2 {family} exact zeros on {dev.type}", ref.BWD_KINDS)
    dWa, dba, dWb, dbb = (got[k][0].cpu() for k in ("dWa", "dba", "dWb", "dbb"))
    assert bool((dWa[da] == 0).all()) and float(dba[da]) == 0.0 and bool((dWb[:, da] == 0).all())
    assert bool((dWb[db] == 0).all()) and float(dbb[db]) == 0.0


@pytest.mark.parametrize("family", ["mfma", "valu"])
def test_tail_all_zero_row(dev, family):
    H1, H2 = TAIL if family == "mfma" else (33, 7)
    got = check_tail(dev, 65, H1, H2, 0, "aligned" if family == "mfma" else "odd", zero_row=64)
    (y1, *_), _, _ = tail_case(65, H1, H2, zero_row=64)
    assert bool((y1[64] == 0).all()) and bool((got["g1"][0][64] == 0).all())
    assert bool(torch.signbit(y1).any()), "no -0.0 among the inputs"


@pytest.mark.parametrize("family", ["mfma", "valu"])
@pytest.mark.parametrize("b3_shift", [5.0, -40.0])
def test_tail_saturated_logits(dev, family, b3_shift):
    """w3 scaled until logits pass +-90 (exp(-|z|) underflows in fp32), b3 moving them: loss and g1 finite and within bound"""
    H1, H2 = TAIL if family == "mfma" else (33, 7)
    kw = dict(w3_scale=1500.0, b3_shift=b3_shift, labels="float01")
    got = check_tail(dev, 193, H1, H2, 0, "aligned" if family == "mfma" else "odd", **kw)
    _, want, _ = tail_case(193, H1, H2, **kw)
    z = want["logits"][0]
    assert float(z.max()) > 90 and float(z.min()) < -90
    assert _finite(got)


# ---- partial sums ------------------------------------------------------------------------------------------------------------
def _expected_G(B, mfma, knob):
    if not mfma:
        return min(-(-B // ML_TS), ML_MAX_WG)
    return min(-(-(-(-B // MM_TS)) // MM_WAVES), min(knob, MM_MAX_WG) if knob > 0 else MM_MAX_WG)


@pytest.mark.parametrize("K0,H1,H2,knob,B", [CRITEO + (0, KNOB_B), CRITEO + (1, KNOB_B), CRITEO + (2, KNOB_B), CRITEO + (-1, KNOB_B),
                                             (5, 33, 7, 0, KNOB_B), CAP_VALU + (0, CAP_B_BWD)])
def test_mlp2_bwd_parts_rows(dev, K0, H1, H2, knob, B):
    """the G rows tzr_mlp2_bwd_parts leaves, [dWb | dbb | dWa | dba]: their float64 column sums within bound of the truth and of
    tzr_mlp2_bwd; G = the tile-derived count"""
    mfma = (K0, H1, H2) == CRITEO and knob >= 0
    place = "aligned" if mfma else "odd"
    ins, want, lit = mlp2_case(B, K0, H1, H2)
    got = _twice(lambda: run_mlp2(dev, *ins, knob=knob, place=place, do=("bwd",), parts=True))
    P = H2 * H1 + H2 + H1 * K0 + H1
    assert (got["G"], got["P"]) == (_expected_G(B, mfma, knob), P)
    sums = got["rows"][0].cpu().double().sum(0)
    cols = {"dWb": (0, H2 * H1), "dbb": (H2 * H1, H2), "dWa": (H2 * H1 + H2, H1 * K0), "dba": (H2 * H1 + H2 + H1 * K0, H1)}
    summed = {k: [sums[a:a + n].reshape(want[k][0].shape)] for k, (a, n) in cols.items()}
    gaps = _judge(summed, want, lit, f"mlp2 parts (B {B}, {K0}, {H1}, {H2}) knob {knob} on {dev.type}", ref.BWD_KINDS)
    ref.check(_twice(lambda: run_mlp2(dev, *ins, knob=knob, place=place, do=("bwd",))), summed, gaps, "tzr_mlp2_bwd against the summed rows", ref.BWD_KINDS)


# ---- what the lists above hold -----------------------------------------------------------------------------------------------
def test_the_shapes_take_both_families_every_tail_and_both_sides_of_each_cap():
    def fwd16(K0, H1, H2):  # mb_fwd16_fits / mlp2_bwd_partials on aligned operands
        return K0 <= 16 and (H1, H2) == CRITEO[1:]

    assert all(fwd16(K0, *CRITEO[1:]) for K0 in MFMA_K0) and not any(fwd16(*s) for s in VALU_SHAPES)
    assert {(17, 64, 16), (13, 63, 16), (13, 64, 15)} <= set(VALU_SHAPES)  # one off the MFMA shape in each dimension
    assert {(64, 31), (63, 32)} <= set(TAIL_VALU_SHAPES) and TAIL not in TAIL_VALU_SHAPES
    assert all(k <= m for s in VALU_SHAPES for k, m in zip(s, ML_MAX)) and ML_MAX in VALU_SHAPES  # the largest the entries take
    assert {1, 16} <= set(MFMA_K0) and any(k % 4 for k in MFMA_K0) and any(k % 4 == 0 for k in MFMA_K0)
    assert any(s[0] % 4 and s[1] % 4 and s[2] % 2 for s in VALU_SHAPES)  # every LDS padding of the general kernels
    # partial and whole tiles, one and several waves / workgroups
    assert {MM_TS - 1, MM_TS, MM_TS + 1} <= set(MFMA_B) and {MM_TS * MM_WAVES - 1, MM_TS * MM_WAVES, MM_TS * MM_WAVES + 1} <= set(MFMA_B)
    assert {ML_TS - 1, ML_TS, ML_TS + 1} <= set(VALU_B) and max(VALU_B) > 2 * ML_TS and 1 in VALU_B and 1 in MFMA_B
    assert max(MFMA_B) > 3 * MM_TS * MM_WAVES and max(MFMA_B) % MM_TS
    # knob 1: every wave of the one workgroup two or more turns, last tile partial
    tiles = -(-KNOB_B // MM_TS)
    assert tiles >= 2 * MM_WAVES and KNOB_B % MM_TS
    # both sides of each cap: every other case is below it, the cap cases one partial tile row past it
    for B, cap in ((CAP_B_BWD, ML_MAX_WG), (CAP_B_FWD, ML_FWD_WG)):
        assert -(-B // ML_TS) > cap and B % ML_TS and -(-B // MM_TS) > cap * MM_WAVES and B % MM_TS
    assert MM_MAX_WG == ML_MAX_WG and MM_FWD_WG == ML_FWD_WG
    assert all(-(-B // MM_TS) <= MM_MAX_WG * MM_WAVES for B in MFMA_B + VALU_B + (KNOB_B, ALIGN_B))
    assert not fwd16(*CAP_VALU) and CAP_VALU[1:] != TAIL
