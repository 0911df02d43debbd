"""The row-streaming glue kernels called directly at their C entry points -- csrc/dense_ops.hip (tzr_relu_bwd_colsum, tzr_head_bwd,
tzr_head_bwd_relu, tzr_skinny_linear_fwd / _bwd and their _parts forms, tzr_bce_logits), csrc/gate_mix.hip (tzr_moe_mix_fwd / _bwd)
and csrc/linear_bwd.hip (tzr_linear_bwd_relu) -- on column slices of wider NaN-filled tensors whose row strides differ from
the slice widths, against the float64 restatement of each operation (tests/dense_glue_ref.py).

Bound, per tensor kind: |ours - fp64| / max(1, |fp64|) <= max(4 x gap, 2^-20), gap = the distance of torch's literal fp32 form
on the CPU to float64 on the same inputs (the rule of tests/test_ln_mask_kernel.py).  Inputs are standard normal and unscaled.
Where the arithmetic is one rounding the result is held bit for bit instead: g of relu_bwd_colsum, gx of head_bwd, g of
head_bwd_relu.  After every call: the padding around each output slice is still NaN, the three guard elements behind each flat
output are still NaN, the documented padding slots inside the flat outputs are exactly 0, and a second run is bit-equal.

The shapes are the smallest that reach each class of the launch geometry; `test_the_cases_reach_every_class_of_the_launch_geometry`
restates that geometry and holds the lists to it.

Measured, the kernels' distance to float64 over the literal form's (printed per case and kind), lane emulator | MI355X:
relu colsum 0.48 - 4.20 | 0.48 - 4.20; head gw 0.02 - 1.00 | 0.06 - 1.00, gb 0.02 - 4.01 | 0.02 - 4.01; head_relu gw 0.14 - 1.22 |
0.04 - 1.00, gb 0.78 - 15.21 | 0.78 - 15.21, colsum 0.25 - 3.84 | 0.25 - 3.84; skinny y 0.19 - 1.30 | 0.22 - 1.00, gx 1.00 | 1.00,
gw 0.24 - 1.20 | 0.06 - 1.20, gb 0.20 - 1.43 | 0.20 - 1.43; moe out 0.76 - 1.12 | 0.72 - 1.00, probs 0.99 - 1.00 | 1.00,
d_logits 0.50 - 1.69 | 0.48 - 1.08, d_expert 0.85 - 1.35 | 0.86 - 1.35; linear_bwd g 0.62 - 3.53 | 0.41 - 1.96, colsum 0.36 - 3.53 |
0.36 - 1.96; bce loss 0.16 - 1.00 | 1.00 - 1.54, B x grad 1.26 - 1.30 | 1.26 - 1.29.  The sums made of fp32 additions alone
(colsum, gb) have the same bits on both: the order of additions is fixed and the emulator runs it as written.
Three figures are above 4, each of them under the 2^-20 floor, which is what holds them: relu colsum 4.20 and head gb 4.01 at
(1000, 12) (errors 8.8e-7 and 5.5e-7), head_relu gb 15.21 at (8197, 512) (8.5e-7 against a literal gap of 5.6e-8: one scalar,
which torch adds pairwise).  The cause is the order of additions: at N = 12 one thread per column adds the sums of all 85
row lanes in one serial chain (dense_ops.hip:168-171, :265-272), and the finish adds the workgroups' rows in sixteen serial
chains (parts_sum.h), where torch's column sum is blocked and pairwise.  head_relu colsum at (1000, 12) is the case nearest
to its bound without the floor: 3.84, error 3.17e-6 against 4 x gap = 3.30e-6.
"""
import ctypes as C

import pytest
import torch

import dense_glue_ref as ref
from torcheasyrec_amd import _lib

NAN = float("nan")
PAD = 4  # columns on either side of a slice: these kernels load and store 16 bytes at a time, a slice starts on a multiple of 4 floats

# the launch geometry, restated (csrc/dense_ops.hip, csrc/gate_mix.hip, csrc/linear_bwd.hip)
RB_THREADS = 256  # dense_ops.hip:125
RB_MAX_WG = 1024  # dense_ops.hip:126
RB_UNROLL = 4  # dense_ops.hip:128
SK_FWD_MAX_WG = 2048  # dense_ops.hip:482
MX_THREADS = 256  # gate_mix.hip:34 (GM_THREADS)
MX_MAX_WG = 4096  # gate_mix.hip:37 (GM_MOE_MAX_GRID)
DN_THREADS, DN_ITEMS, DN_MAX_PARTS = 256, 4, 4096  # dense_ops.hip:19-21
LB_TS = 16  # linear_bwd.hip:32
WAVE = 64

# (B, N) of relu_bwd_colsum, head_bwd, head_bwd_relu
RB_CASES = [
    (1, 4),
    (5, 12),  # N4 = 3, rl = 85: thread 255 idle
    (1000, 12),
    (257, 256),
    (777, 200),  # N4 = 50, rl = 5: 6 idle threads
    (300, 516),  # N4 = 129, rl = 1: 127 idle threads
    (999, 1020),  # N4 = 255
    (4101, 1024),  # past the cap: 8 rows per workgroup, 513 workgroups, the last has 5 rows
    (8197, 512),  # past the cap: 16 rows per workgroup, 513 workgroups, the last has 5 rows
    (61500, 68),  # rl = 15; past the cap: 120 rows per workgroup, 513 workgroups, the last has 60 rows (its loop runs once, the others' twice)
]
# (B, K, n_out) of the skinny linear
SK_CASES = [
    (1, 4, 1),
    (100, 12, 5),  # K/4 = 3 < lgp = 4
    (37, 200, 6),
    (513, 260, 2),  # K/4 = 65 > 64: a lane walks its columns, one of them twice
    (300, 512, 4),
    (999, 1020, 7),
    (4101, 1024, 3),  # backward past the cap
    (61500, 68, 8),  # backward past the cap, 8 outputs
    (65569, 128, 3),  # forward past its cap: 32 rows per workgroup x 2048 = 65536, 33 rows in the second pass
]
# (B, H, E, T) of the MoE mix: the nine <TT, EE> instantiations first
MX_CASES = [
    (70, 12, 1, 1), (33, 36, 3, 1), (33, 100, 8, 1),
    (33, 68, 2, 2), (70, 20, 3, 2), (33, 8, 7, 2),
    (33, 16, 2, 4), (33, 132, 4, 4), (70, 200, 5, 3),
    (1, 4, 1, 1),
    (70, 264, 3, 2),  # H/4 = 66 > 64
    (70, 1024, 3, 2),
    (32769, 128, 2, 1),  # past the cap: 8 rows per workgroup x 4096 = 32768, one row left: wave 0's second iteration has one lane group on, one off
    (16387, 256, 2, 1),  # past the cap with one row per wave
]
# (N, K, H, cap) of linear_bwd_relu: every <KS, HB>; cap = tzr_tune("linear_bwd_wg")
LB_CASES = [(N, K, H, 0) for K in (16, 32, 64) for H in (64, 128, 256) for N in (1, 37, 515)] + [(515, 64, 256, 3)]  # 33 tiles over 3 workgroups
BCE_B = DN_MAX_PARTS * DN_THREADS * DN_ITEMS + 5  # the smallest batch that takes the per_wg branch
BCE_CASES = [("float32", False), ("int32", True), ("int64", False)]


def rb_geometry(B, N):
    """dense_ops.hip:191-198 (and :292-298, :390-396, :585-591)"""
    N4 = N // 4
    rl = RB_THREADS // N4
    rows = rl * RB_UNROLL
    raw = -(-B // rows)
    n_wg = raw
    if raw > RB_MAX_WG:
        rows = -(-(-(-B // RB_MAX_WG)) // (rl * RB_UNROLL)) * (rl * RB_UNROLL)
        n_wg = -(-B // rows)
    return {"N4": N4, "rl": rl, "idle": RB_THREADS - rl * N4, "raw_wg": raw, "rows_per_wg": rows, "n_wg": n_wg, "last": B - (n_wg - 1) * rows}


def lane_group(n4):
    """dense_ops.hip:478-479, gate_mix.hip:213-214: the smallest power of two >= n4, at most a wave"""
    lgp = 1
    while lgp < n4 and lgp < WAVE:
        lgp <<= 1
    return lgp


def sk_fwd_geometry(B, K):
    """dense_ops.hip:478-482"""
    lgp = lane_group(K // 4)
    rows = (WAVE // lgp) * RB_UNROLL * (RB_THREADS // WAVE)
    return {"lgp": lgp, "rows_per_wg": rows, "raw_wg": -(-B // rows)}


def mx_geometry(B, H):
    """gate_mix.hip:212-219 (gm_geometry at GM_MOE_MAX_GRID)"""
    lgp = lane_group(H // 4)
    rows = (WAVE // lgp) * (MX_THREADS // WAVE)
    return {"lgp": lgp, "rows_per_wg": rows, "raw_wg": -(-B // rows)}


def mx_dispatch(E, T):
    """gate_mix.hip:198-210 (GM_DISPATCH), :253-254 (the classes of tzr_moe_mix_*)"""
    return (1 if T <= 1 else 2 if T <= 2 else 4), (2 if E <= 2 else 4 if E <= 4 else 8)


def bce_geometry(B):
    """dense_ops.hip:100-106"""
    tile = DN_THREADS * DN_ITEMS
    raw = -(-B // tile)
    per_wg, n_wg = tile, raw
    if raw > DN_MAX_PARTS:
        per_wg = -(-(-(-B // DN_MAX_PARTS)) // tile) * tile
        n_wg = -(-B // per_wg)
    return {"raw_wg": raw, "per_wg": per_wg, "n_wg": n_wg, "last": B - (n_wg - 1) * per_wg}


def sk_row_len(K, n):
    return n * K + (n + 3) // 4 * 4  # dense_ops.hip:566


def test_the_cases_reach_every_class_of_the_launch_geometry():
    """the comments of the lists above, asserted: a later edit of a list cannot drop a class silently"""
    geo = {c: rb_geometry(*c) for c in RB_CASES}
    assert (geo[(5, 12)]["rl"], geo[(5, 12)]["idle"]) == (85, 1)
    assert (geo[(777, 200)]["rl"], geo[(777, 200)]["idle"]) == (5, 6)
    assert (geo[(300, 516)]["rl"], geo[(300, 516)]["idle"]) == (1, 127)
    assert geo[(999, 1020)]["N4"] == 255
    past = {c: g for c, g in geo.items() if g["raw_wg"] > RB_MAX_WG}
    assert {c: (g["rows_per_wg"], g["n_wg"], g["last"]) for c, g in past.items()} == {
        (4101, 1024): (8, 513, 5), (8197, 512): (16, 513, 5), (61500, 68): (120, 513, 60)}
    assert geo[(61500, 68)]["rl"] == 15 and geo[(61500, 68)]["last"] <= 15 * RB_UNROLL < geo[(61500, 68)]["rows_per_wg"]
    assert any(RB_THREADS % g["N4"] != 0 for g in past.values()) and any(RB_THREADS % g["N4"] == 0 for g in past.values())
    assert sum(RB_THREADS % g["N4"] != 0 for g in geo.values()) >= 4
    assert all(g["n_wg"] <= RB_MAX_WG for g in geo.values())
    # the skinny backward has the RB geometry over (B, K); every instantiation of its n_out ladder (1, 2, <= 4, <= 8) is there
    skb = {c: rb_geometry(c[0], c[1]) for c in SK_CASES}
    assert {c for c, g in skb.items() if g["raw_wg"] > RB_MAX_WG} >= {(4101, 1024, 3), (61500, 68, 8)}
    assert any(RB_THREADS % g["N4"] != 0 for g in skb.values())
    assert {1 if n == 1 else 2 if n == 2 else 4 if n <= 4 else 8 for _, _, n in SK_CASES} == {1, 2, 4, 8}
    skf = {c: sk_fwd_geometry(c[0], c[1]) for c in SK_CASES}
    assert skf[(100, 12, 5)]["lgp"] == 4 > 12 // 4
    assert any(K // 4 > WAVE for _, K, _ in SK_CASES)
    g = skf[(65569, 128, 3)]
    assert g["raw_wg"] > SK_FWD_MAX_WG and g["rows_per_wg"] == 32 and 65569 - 32 * SK_FWD_MAX_WG == 33
    # MoE: all nine <TT, EE>, a row narrower than its lane group, one wider than a wave, both caps
    assert {mx_dispatch(E, T) for _, _, E, T in MX_CASES[:9]} == {(tt, ee) for tt in (1, 2, 4) for ee in (2, 4, 8)}
    mx = {c: mx_geometry(c[0], c[1]) for c in MX_CASES}
    assert sum(c[1] // 4 < g["lgp"] for c, g in mx.items()) >= 5 and any(c[1] // 4 > WAVE for c in mx)
    g = mx[(32769, 128, 2, 1)]
    assert g["raw_wg"] > MX_MAX_WG and g["rows_per_wg"] == 8 and 32769 - 8 * MX_MAX_WG == 1 and WAVE // g["lgp"] == 2
    g = mx[(16387, 256, 2, 1)]
    assert g["raw_wg"] > MX_MAX_WG and g["rows_per_wg"] == 4 and WAVE // g["lgp"] == 1
    assert all(E > 1 and B > 10 for B, _, E, _ in MX_CASES[-2:])  # the extreme logit rows go through the grid-stride loop too
    # linear_bwd_relu: every <KS, HB> at one row, a partial tile and more tiles than one; the capped run walks 11 tiles a workgroup
    assert {(K // 4, H // 64) for _, K, H, _ in LB_CASES} == {(ks, hb) for ks in (4, 8, 16) for hb in (1, 2, 4)}
    for K in (16, 32, 64):
        for H in (64, 128, 256):
            assert {N for N, k, h, cap in LB_CASES if (k, h, cap) == (K, H, 0)} == {1, 37, 515}
    assert [(-(-N // LB_TS), cap) for N, _, _, cap in LB_CASES if cap] == [(33, 3)]
    g = bce_geometry(BCE_B)
    assert g["raw_wg"] == DN_MAX_PARTS + 1 and (g["per_wg"], g["n_wg"], g["last"]) == (2048, 2049, 5)
    assert bce_geometry(BCE_B - 5)["raw_wg"] == DN_MAX_PARTS  # one logit fewer than the +5 tail's first: the plain branch
    assert {k for k, _ in BCE_CASES} == {"float32", "int32", "int64"} and any(w for _, w in BCE_CASES)


def _wide(t, dev, extra=0):
    """the [B, n] tensor `t` as the column slice [PAD, PAD + n) of a NaN-filled [B, n + 2 PAD + extra] one -> (wide, slice)"""
    w, v = _blank(t.shape[0], t.shape[1], dev, extra)
    v.copy_(t)
    return w, v


def _blank(B, n, dev, extra=0):
    assert extra % 4 == 0
    w = torch.full((B, n + 2 * PAD + extra), NAN, dtype=torch.float32, device=dev)
    v = w[:, PAD:PAD + n]
    assert v.data_ptr() % 16 == 0 and w.stride(0) % 4 == 0 and w.stride(0) != n
    return w, v


def _cols(t, dev, width, at):
    """the [B, n] tensor `t` (or n columns of NaN for an int `t`) at column `at` of a NaN-filled [B, width] one"""
    B, n = (t.shape if torch.is_tensor(t) else t)
    w = torch.full((B, width), NAN, dtype=torch.float32, device=dev)
    v = w[:, at:at + n]
    if torch.is_tensor(t):
        v.copy_(t)
    return w, v


def _untouched(w, v):
    """nothing of the wide tensor `w` outside its slice `v` was written"""
    at = v.storage_offset() - w.storage_offset()
    n = v.shape[1]
    return bool(torch.isnan(w[:, :at]).all()) and bool(torch.isnan(w[:, at + n:]).all())


def _flat(n, dev):
    """a flat output of n floats with three guard elements behind it, all NaN"""
    return torch.full((n + 3,), NAN, dtype=torch.float32, device=dev)


def _guarded(f, n):
    return f.numel() == n + 3 and bool(torch.isnan(f[n:]).all())


def _zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


def _rows(ws, G, P):
    """the G rows of P partial sums a _parts entry point leaves at the head of its workspace"""
    return ws[:G * P * 4].clone().view(torch.float32).view(G, P)


def _bit_equal(a, b):
    return a.keys() == b.keys() and all(len(a[k]) == len(b[k]) and all(torch.equal(p, q) for p, q in zip(a[k], b[k])) for k in a)


def _hold(got, want, lit, kinds, what):
    gaps = ref.gaps(lit, want, kinds)
    for k in kinds:
        if gaps[k] > 0:
            print(f"{what} {k}: ours / literal {ref.rel_err(got[k], want[k]) / gaps[k]:.2f}")
    ref.check(got, want, gaps, what, kinds)
    return gaps


# ---- relu_bwd_colsum ----------------------------------------------------------------------------------------------------------

def run_relu(dev, gy, y, parts=False):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    B, N = y.shape
    _, gv = _wide(gy, dev, 0)
    _, yv = _wide(y, dev, 4)
    ow, ov = _blank(B, N, dev, 8)
    ws = _lib.workspace(lib.tzr_relu_bwd_colsum_workspace(B, N), dev)
    if parts:
        G = C.c_int(-1)
        assert lib.tzr_relu_bwd_colsum_parts(p(gv), gv.stride(0), p(yv), yv.stride(0), B, N, p(ov), ov.stride(0), p(ws), ws.numel(), C.byref(G), st) == 0
        assert _untouched(ow, ov)
        return {"g": [ov], "rows": [_rows(ws, G.value, N)]}
    col = _flat(N, dev)
    assert lib.tzr_relu_bwd_colsum(p(gv), gv.stride(0), p(yv), yv.stride(0), B, N, p(ov), ov.stride(0), p(col), p(ws), ws.numel(), st) == 0
    assert _untouched(ow, ov) and _guarded(col, N)
    return {"g": [ov], "colsum": [col[:N]]}


@pytest.mark.parametrize("B,N", RB_CASES)
def test_relu_bwd_colsum(dev, B, N):
    gy, y = ref.draw_relu(B, N, seed=B * 131 + N)
    what = f"relu ({B}, {N}) on {dev.type}"
    want, lit = ref.relu_bwd_colsum_literal(gy, y), ref.relu_bwd_colsum_literal(gy, y, dtype=torch.float32)
    got = run_relu(dev, gy, y)
    assert torch.equal(got["g"][0].cpu(), torch.where(y > 0, gy, torch.zeros(())))  # one operation: exact
    gaps = _hold(got, want, lit, ref.RELU_KINDS, what)
    assert _bit_equal(got, run_relu(dev, gy, y)), "two runs of the same case differ"
    geo = rb_geometry(B, N)
    if geo["raw_wg"] > RB_MAX_WG:  # the rows tzr_relu_bwd_colsum_parts leaves, added in float64, under the same bound
        parts = run_relu(dev, gy, y, parts=True)
        assert torch.equal(parts["g"][0], got["g"][0]) and tuple(parts["rows"][0].shape) == (geo["n_wg"], N)
        ref.check({"colsum": [parts["rows"][0].cpu().double().sum(0)]}, want, gaps, what + " parts", ref.RELU_KINDS)


# ---- the one-unit head ----------------------------------------------------------------------------------------------------------

def run_head(dev, gy, x, w, relu=False, need_gx=True):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    B, N = x.shape
    gyw, gyv = _cols(gy.reshape(B, 1), dev, 5, 2)  # a per-row scalar: stride 5
    _, xv = _wide(x, dev, 4)
    wd = w.to(dev).contiguous()
    ow, ov = _blank(B, N, dev, 12)
    if relu:
        sums = _flat(2 * N + 4, dev)
        ws = _lib.workspace(lib.tzr_head_bwd_relu_workspace(B, N), dev)
        assert lib.tzr_head_bwd_relu(p(gyv), gyw.stride(0), p(xv), xv.stride(0), p(wd), B, N, p(ov), ov.stride(0), p(sums), p(ws), ws.numel(), st) == 0
        assert _untouched(ow, ov) and _guarded(sums, 2 * N + 4) and _zero(sums[N + 1:N + 4])
        return {"g": [ov], "gw": [sums[:N]], "gb": [sums[N:N + 1]], "colsum": [sums[N + 4:2 * N + 4]]}
    wb = _flat(N + 4, dev)
    ws = _lib.workspace(lib.tzr_head_bwd_workspace(B, N), dev)
    assert lib.tzr_head_bwd(p(gyv), gyw.stride(0), p(xv), xv.stride(0), p(wd), B, N, p(ov) if need_gx else None, ov.stride(0) if need_gx else 0,
                            p(wb), p(ws), ws.numel(), st) == 0
    assert _guarded(wb, N + 4) and _zero(wb[N + 1:N + 4])
    assert _untouched(ow, ov) if need_gx else bool(torch.isnan(ow).all())
    return {"gx": [ov], "gw": [wb[:N]], "gb": [wb[N:N + 1]]}


@pytest.mark.parametrize("B,N", RB_CASES)
def test_head_bwd(dev, B, N):
    gy, x, w = ref.draw_head(B, N, seed=B * 137 + N)
    what = f"head ({B}, {N}) on {dev.type}"
    want, lit = ref.head_bwd_literal(gy, x, w), ref.head_bwd_literal(gy, x, w, dtype=torch.float32)
    got = run_head(dev, gy, x, w)
    assert torch.equal(got["gx"][0].cpu(), gy[:, None] * w[None, :])  # one fp32 product: exact
    _hold(got, want, lit, ref.HEAD_KINDS, what)
    assert _bit_equal(got, run_head(dev, gy, x, w)), "two runs of the same case differ"
    bare = run_head(dev, gy, x, w, need_gx=False)  # d_grad_x = NULL: the sums are the same additions
    assert torch.equal(bare["gw"][0], got["gw"][0]) and torch.equal(bare["gb"][0], got["gb"][0])


@pytest.mark.parametrize("B,N", RB_CASES)
def test_head_bwd_relu(dev, B, N):
    gy, x, w = ref.draw_head(B, N, seed=B * 139 + N, relu=True)
    what = f"head_relu ({B}, {N}) on {dev.type}"
    want, lit = ref.head_bwd_relu_literal(gy, x, w), ref.head_bwd_relu_literal(gy, x, w, dtype=torch.float32)
    got = run_head(dev, gy, x, w, relu=True)
    assert torch.equal(got["g"][0].cpu(), torch.where(x > 0, gy[:, None] * w[None, :], torch.zeros(())))  # one fp32 product, masked: exact
    _hold(got, want, lit, ref.HEAD_RELU_KINDS, what)
    assert _bit_equal(got, run_head(dev, gy, x, w, relu=True)), "two runs of the same case differ"


# ---- the skinny linear ----------------------------------------------------------------------------------------------------------

def run_skinny(dev, x, w, b, gy, need_gx=True, parts=False):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    (B, K), n = x.shape, w.shape[0]
    _, xv = _wide(x, dev, 4)
    _, wv = _wide(w, dev, 0)  # [n, K + 8]
    bd = None if b is None else b.to(dev)
    yw, yv = _cols((B, n), dev, n + 5, 2)
    gyw, gyv = _cols(gy, dev, n + 5, 3)
    gxw, gxv = _blank(B, K, dev, 8)
    if not parts:
        assert lib.tzr_skinny_linear_fwd(p(xv), xv.stride(0), p(wv), wv.stride(0), p(bd), B, K, n, p(yv), yw.stride(0), st) == 0
    assert _untouched(yw, yv)
    P = sk_row_len(K, n)
    ws = _lib.workspace(lib.tzr_skinny_linear_bwd_workspace(B, K, n), dev)
    gx_args = (p(gxv), gxv.stride(0)) if need_gx else (None, 0)
    if parts:
        G, Pg = C.c_int(-1), C.c_int(-1)
        assert lib.tzr_skinny_linear_bwd_parts(p(gyv), gyw.stride(0), p(xv), xv.stride(0), p(wv), wv.stride(0), B, K, n, *gx_args, p(ws), ws.numel(),
                                               C.byref(G), C.byref(Pg), st) == 0
        assert Pg.value == P
        out = {"rows": [_rows(ws, G.value, P)]}
    else:
        wb = _flat(P, dev)
        assert lib.tzr_skinny_linear_bwd(p(gyv), gyw.stride(0), p(xv), xv.stride(0), p(wv), wv.stride(0), B, K, n, *gx_args, p(wb), p(ws), ws.numel(),
                                         st) == 0
        assert _guarded(wb, P) and _zero(wb[n * K + n:P])
        out = {"gw": [wb[:n * K].view(n, K)], "gb": [wb[n * K:n * K + n]]}
    assert _untouched(gxw, gxv) if need_gx else bool(torch.isnan(gxw).all())
    return {"y": [yv], "gx": [gxv], **out}


@pytest.mark.parametrize("B,K,n", SK_CASES)
def test_skinny_linear(dev, B, K, n):
    x, w, b, gy = ref.draw_skinny(B, K, n, seed=B * 149 + K * 7 + n)
    what = f"skinny ({B}, {K}, {n}) on {dev.type}"
    want, lit = ref.skinny_linear_literal(x, w, b, gy), ref.skinny_linear_literal(x, w, b, gy, dtype=torch.float32)
    got = run_skinny(dev, x, w, b, gy)
    gaps = _hold(got, want, lit, ref.SKINNY_KINDS, what)
    assert _bit_equal(got, run_skinny(dev, x, w, b, gy)), "two runs of the same case differ"
    geo = rb_geometry(B, K)
    if geo["raw_wg"] > RB_MAX_WG:  # the rows tzr_skinny_linear_bwd_parts leaves, added in float64, under the same bound
        rows = run_skinny(dev, x, w, b, gy, parts=True)["rows"][0]
        assert tuple(rows.shape) == (geo["n_wg"], sk_row_len(K, n)) and _zero(rows[:, n * K + n:])
        total = rows.cpu().double().sum(0)
        ref.check({"gw": [total[:n * K].view(n, K)], "gb": [total[n * K:n * K + n]]}, want, gaps, what + " parts", ("gw", "gb"))


@pytest.mark.parametrize("B,K,n", SK_CASES)
def test_skinny_linear_without_bias_and_input_gradient(dev, B, K, n):
    """bias = NULL in the forward, d_grad_x = NULL in the backward"""
    x, w, b, gy = ref.draw_skinny(B, K, n, seed=B * 149 + K * 7 + n)
    what = f"skinny_bare ({B}, {K}, {n}) on {dev.type}"
    kinds = ("y", "gw", "gb")
    want, lit = ref.skinny_linear_literal(x, w, None, gy), ref.skinny_linear_literal(x, w, None, gy, dtype=torch.float32)
    got = run_skinny(dev, x, w, None, gy, need_gx=False)
    _hold(got, want, lit, kinds, what)


# ---- the MoE mix ----------------------------------------------------------------------------------------------------------

def run_moe(dev, xs, ls, gos):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    (B, H), E, T = xs[0].shape, len(xs), len(ls)
    m = _lib.TzrMoeMix()
    m.B, m.H, m.n_experts, m.n_tasks = B, H, E, T
    keep, outs = [], {"out": [], "probs": [], "d_logits": [], "d_expert": []}
    for e, x in enumerate(xs):
        xw, xv = _wide(x, dev, 4 * (e % 3))
        dw, dv = _blank(B, H, dev, 4 * ((e + 1) % 3) + 12)
        m.expert[e], m.expert_stride[e], m.d_expert[e], m.d_expert_stride[e] = p(xv), xv.stride(0), p(dv), dv.stride(0)
        keep += [xw, (dw, dv)]
        outs["d_expert"].append(dv)
    for t in range(T):
        lw, lv = _cols(ls[t], dev, E + 3, 1)
        dlw, dlv = _cols((B, E), dev, E + 3, 1)
        ow, ov = _blank(B, H, dev, 4 * t + 24)
        gw, gv = _wide(gos[t], dev, 4 * t + 40)
        probs = torch.full((B, E), NAN, dtype=torch.float32, device=dev)  # contiguous, as the header says
        m.logits[t], m.logits_stride[t], m.probs[t] = p(lv), lw.stride(0), p(probs)
        m.out[t], m.out_stride[t] = p(ov), ov.stride(0)
        m.grad_out[t], m.grad_out_stride[t] = p(gv), gv.stride(0)
        m.d_logits[t], m.d_logits_stride[t] = p(dlv), dlw.stride(0)
        keep += [lw, gw, (dlw, dlv), (ow, ov)]
        outs["out"].append(ov)
        outs["probs"].append(probs)
        outs["d_logits"].append(dlv)
    assert lib.tzr_moe_mix_fwd(C.byref(m), st) == 0
    assert lib.tzr_moe_mix_bwd(C.byref(m), st) == 0
    assert all(_untouched(*k) for k in keep if isinstance(k, tuple))
    return outs


@pytest.mark.parametrize("B,H,E,T", MX_CASES)
def test_moe_mix(dev, B, H, E, T):
    xs, ls, gos = ref.draw_moe(B, H, E, T, seed=B * 151 + H * 11 + E * 5 + T)
    what = f"moe ({B}, {H}, {E}, {T}) on {dev.type}"
    want, lit = ref.moe_mix_literal(xs, ls, gos), ref.moe_mix_literal(xs, ls, gos, dtype=torch.float32)
    assert all(bool(torch.isfinite(t).all()) for k in ref.MOE_KINDS for t in want[k])
    got = run_moe(dev, xs, ls, gos)
    _hold(got, want, lit, ref.MOE_KINDS, what)
    assert _bit_equal(got, run_moe(dev, xs, ls, gos)), "two runs of the same case differ"


# ---- linear_bwd_relu ----------------------------------------------------------------------------------------------------------

def run_linear_bwd(dev, gin, W, y, cap):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    (N, K), H = gin.shape, W.shape[1]
    _, gv = _wide(gin, dev, 4)
    _, Wv = _wide(W, dev, 0)  # [K, H + 8]
    _, yv = _wide(y, dev, 8)
    ow, ov = _blank(N, H, dev, 12)
    col = _flat(H, dev)
    ws = _lib.workspace(lib.tzr_linear_bwd_relu_workspace(N, H), dev)
    assert lib.tzr_linear_bwd_relu_supported(K, H) == 1
    assert lib.tzr_tune(b"linear_bwd_wg", cap) == 0  # (put back by conftest's _default_knobs)
    assert lib.tzr_linear_bwd_relu(p(gv), gv.stride(0), p(Wv), Wv.stride(0), p(yv), yv.stride(0), N, K, H, p(ov), ov.stride(0), p(col), p(ws),
                                   ws.numel(), st) == 0
    assert _untouched(ow, ov) and _guarded(col, H)
    return {"g": [ov], "colsum": [col[:H]]}


@pytest.mark.parametrize("N,K,H,cap", LB_CASES)
def test_linear_bwd_relu(dev, N, K, H, cap):
    gin, W, y = ref.draw_linear_bwd(N, K, H, seed=N * 157 + K * 3 + H)
    what = f"linear_bwd ({N}, {K}, {H}, cap {cap}) on {dev.type}"
    want, lit = ref.linear_bwd_relu_literal(gin, W, y), ref.linear_bwd_relu_literal(gin, W, y, dtype=torch.float32)
    got = run_linear_bwd(dev, gin, W, y, cap)
    assert torch.equal(got["g"][0].cpu() != 0, want["g"][0] != 0)  # the mask is y's, exactly
    _hold(got, want, lit, ref.LINEAR_BWD_KINDS, what)
    assert _bit_equal(got, run_linear_bwd(dev, gin, W, y, cap)), "two runs of the same case differ"


# ---- BCE with logits ----------------------------------------------------------------------------------------------------------

def run_bce(dev, x, y, w):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    B = x.numel()
    xd, yd, wd = x.to(dev), y.to(dev), None if w is None else w.to(dev)
    loss, grad = _flat(1, dev), _flat(B, dev)
    ws = _lib.workspace(lib.tzr_bce_logits_workspace(B), dev)
    assert lib.tzr_bce_logits(p(xd), p(yd), yd.element_size(), int(yd.is_floating_point()), p(wd), B, p(loss), p(grad), p(ws), ws.numel(), st) == 0
    assert _guarded(loss, 1) and _guarded(grad, B)
    return {"loss": [loss[:1]], "grad": [grad[:B]]}


@pytest.mark.parametrize("label_kind,weighted", BCE_CASES)
def test_bce_logits_past_the_partial_sum_cap(dev, label_kind, weighted):
    """B = 4096 x 1024 + 5, the only size class with several tiles per workgroup: 2049 workgroups of 2048 logits, the last has 5"""
    x, y, w = ref.draw_bce(BCE_B, label_kind, weighted, seed=len(label_kind) + 2 * weighted)
    what = f"bce ({label_kind}{', weighted' if weighted else ''}) on {dev.type}"
    want, lit = ref.bce_logits_literal(x, y, w), ref.bce_logits_literal(x, y, w, dtype=torch.float32)
    got = run_bce(dev, x, y, w)
    scaled = {"loss": got["loss"], "grad": [got["grad"][0].cpu().double() * BCE_B]}
    _hold(scaled, want, lit, ref.BCE_KINDS, what)
    assert _bit_equal(got, run_bce(dev, x, y, w)), "two runs of the same case differ"
