"""DIN target attention on the jagged positions (csrc/din_attention.hip, jagged_ops.hip, gemm_rows.hip, linear_bwd.hip) at the
lengths, widths and batches of BASELINE config 4 (multi_tower_din) and at the edges where the kernels branch: per-sample loops
that stride by the wave (second pass past 64 positions), column loops that stride by 16 float4s (second pass past 64 floats),
the assemble backward's position groups (64 / (D / 4), uneven at D = 20, 68, 252), and the grid-stride loops past the grid caps.

Reference: oracle.tzrec_oracle.din_encoder -- the reference's DINEncoder.forward with the literal [q, k, q - k, q * k] input on the
padded tensor -- in float64, differentiated by autograd: the output, the query gradient, every row's gradient, every attention-MLP
and score-layer gradient.

Bound, per checked tensor t: |got - want| <= TOL * S_t + 1e-7, S_t = max |want_t|, TOL = 1e-5.  Every quantity is a chain of
fp32 sums (contractions of at most 4 D + 2 H <= 1 536 terms, softmax and weighted sums over <= 2 048 positions, weight-gradient
sums over all rows) evaluated in another order than the reference's; a reordered fp32 sum of terms of magnitude m has an error
of a few ulps of m times sqrt(terms) for random data (eps32 = 6e-8, sqrt(2 048) = 45: ~3e-6), and the chain through the MLP and
the softmax compounds a few of them.  One exception: the score layer's bias gradient is sum_n ds_n = 0 exactly (a softmax does
not see a shift of its scores), so its scale is the bound sum_b 2 |g_b|_1 max |k| on sum_n |ds_n|.  The fp32 padded form
(DINEncoder.forward) passes the same bound.  The rows are drawn clear of the ReLU kinks (_clear_of_relu_kinks).  Both stay below 1e-6 S_t on the lane emulator; a loop that drops or repeats a
pass is off by O(S_t).
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle import tzrec_oracle as orc  # noqa: E402
from torcheasyrec_amd import _lib, dense  # noqa: E402
from torcheasyrec_amd.sequence import DIN_JAGGED_MAX_LEN, DINEncoder, _DinTowerFn, jagged_to_padded_dense, segment_reduce  # noqa: E402

TOL = 1e-5
UNSUPPORTED = -4  # TZR_ERR_UNSUPPORTED


def _offsets(lens, dev):
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.as_tensor(lens, dtype=torch.int64), 0)
    return off.to(dev)


def _pad(v, lens, L):
    """[N, D] rows -> [B, L, D], zeros behind a sample's length, rows behind L dropped; differentiable, on v's device and dtype"""
    B, D = lens.numel(), v.shape[1]
    if v.shape[0] == 0 or B == 0 or L == 0:
        return v.new_zeros(B, L, D) + v.sum() * 0
    off = torch.cumsum(lens, 0) - lens
    pos = torch.arange(L, device=v.device)
    valid = pos.unsqueeze(0) < lens.unsqueeze(1)
    idx = torch.where(valid, off.unsqueeze(1) + pos.unsqueeze(0), torch.zeros_like(off).unsqueeze(1))
    return v[idx.reshape(-1)].reshape(B, L, D) * valid.unsqueeze(2).to(v.dtype)


def _names(enc):
    return ["out", "d query", "d rows"] + [n for n, _ in enc.named_parameters()]


def _reference(enc, q, v, lens, max_len, gw):
    """float64 oracle on the inputs' device: [out, d query, d rows, d every parameter] in _names order"""
    dd = torch.float64
    qr, vr = q.detach().to(dd).requires_grad_(True), v.detach().to(dd).requires_grad_(True)
    P = {n: p_.detach().to(dd).requires_grad_(True) for n, p_ in enc.named_parameters()}
    layers = [(P[n], P[n[:-len("weight")] + "bias"]) for n in P if n.startswith("mlp.") and n.endswith(".weight")]
    out = orc.din_encoder(qr, _pad(vr, lens, max_len), lens, layers, (P["linear.weight"], P["linear.bias"]),
                          max_seq_length=enc._max_seq_length)
    ins = [qr, vr] + list(P.values())
    grads = torch.autograd.grad((out * gw.to(dd)).sum(), ins, allow_unused=True)
    return [out.detach()] + [g if g is not None else torch.zeros_like(t) for g, t in zip(grads, ins)]


def _product(enc, q, v, off, lens, max_len, gw, form, row_bucket=1):
    for p_ in enc.parameters():
        p_.grad = None
    qj, vj = q.clone().requires_grad_(True), v.clone().requires_grad_(True)
    if form == "jagged":
        enc.row_bucket = row_bucket
        out = enc.forward_jagged(qj, vj, off, max_len)
    else:
        out = enc({"seq.query": qj, "seq.sequence": _pad(vj, lens, max_len), "seq.sequence_length": lens})
    (out * gw).sum().backward()
    gs = [p_.grad if p_.grad is not None else torch.zeros_like(p_) for p_ in enc.parameters()]
    return [out.detach(), qj.grad, vj.grad] + [g.detach().clone() for g in gs]


def _close(got, want, scale, name):
    err = float((got.double() - want).abs().max()) if want.numel() else 0.0
    assert err <= TOL * scale + 1e-7, f"{name}: max error {err:.3g}, scale {scale:.3g} (bound {TOL * scale + 1e-7:.3g})"


def _clear_of_relu_kinks(enc, q, v, lens, gen, t=1e-5):
    """v with every row redrawn whose hidden pre-activations (float64) come within t * (|x| |W| + |b|) of 0: ReLU has no
    derivative there, and an fp32 evaluation may land on the other side -- a whole term of the gradient, not a rounding error.
    (At B = 8 192 x 50 rows x 256 units a handful of units do; 1e-5 is ~10x the fp32 error of a pre-activation.)"""
    D = v.shape[1]
    qp = torch.nn.functional.pad(q.double(), (0, D - q.shape[1]))
    seg = torch.repeat_interleave(torch.arange(len(lens)), torch.from_numpy(lens)).to(v.device)
    rows = torch.arange(v.shape[0], device=v.device)
    for _ in range(30):
        if rows.numel() == 0:
            return v
        qq, k = qp[seg[rows]], v[rows].double()
        x, bad = torch.cat([qq, k, qq - k, qq * k], dim=1), torch.zeros(rows.numel(), dtype=torch.bool, device=v.device)
        for m in enc.mlp.linears():
            W, b = m.weight.detach().double(), m.bias.detach().double()
            z = x @ W.t() + b
            bad |= (z.abs() <= t * (x.abs() @ W.abs().t() + b.abs())).any(dim=1)
            x = torch.relu(z)
        rows = rows[bad]
        v = v.clone()
        v[rows] = torch.randn(rows.numel(), D, generator=gen).to(v.device)
    raise AssertionError("rows keep landing next to a ReLU kink")


def _check(dev, D, hidden, lens, max_len, qd=None, msl=0, row_bucket=1, own=None, seed=0, padded=True):
    """one batch through forward_jagged (and the fp32 padded form) against the float64 reference; returns the jagged results"""
    qd = qd or D
    torch.manual_seed(seed)
    enc = DINEncoder(D, qd, "seq", {"hidden_units": list(hidden)}, max_seq_length=msl).to(dev)
    assert enc.jagged_capable()
    lens = np.asarray(lens, dtype=np.int64)
    B, N = len(lens), int(lens.sum())
    g = torch.Generator().manual_seed(seed + 1)
    q, v, gw = torch.randn(B, qd, generator=g).to(dev), torch.randn(N, D, generator=g).to(dev), torch.randn(B, D, generator=g).to(dev)
    v = _clear_of_relu_kinks(enc, q, v, lens, g)
    off, lt = _offsets(lens, dev), torch.from_numpy(lens).to(dev)
    want = _reference(enc, q, v, lt, max_len, gw)
    calls0 = _DinTowerFn.own_calls
    got = _product(enc, q, v, off, lt, max_len, gw, "jagged", row_bucket)
    if own is not None:
        assert (_DinTowerFn.own_calls > calls0) == own, "the MLP took the other path"
    forms = {"jagged": got}
    if padded and B:
        forms["padded fp32"] = _product(enc, q, v, off, lt, max_len, gw, "padded")
    kmax = float(v.abs().max()) if N else 0.0
    for form, res in forms.items():
        for name, a_, w_ in zip(_names(enc), res, want):
            scale = float(gw.abs().sum(1).sum()) * 2 * kmax if name == "linear.bias" else (float(w_.abs().max()) if w_.numel() else 0.0)
            _close(a_, w_, scale, f"{form} {name}")
    # positions behind the cut (max_len, max_seq_length) do not exist: their rows get exactly zero gradient; no position: output 0
    cut = min(max_len, msl) if msl > 0 else max_len
    o = np.concatenate([[0], np.cumsum(lens)])
    dv = got[2].cpu()
    for b in np.nonzero(lens > cut)[0]:
        assert bool((dv[o[b] + cut:o[b + 1]] == 0).all()), f"sample {b}: rows behind position {cut} got a gradient"
    empty = torch.from_numpy(lens == 0)
    assert bool((got[0].cpu()[empty] == 0).all())
    return got


# ---- lengths ------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 2047, 2048]


@pytest.mark.parametrize("path", ["library", "own"])
def test_lengths_around_the_wave_and_the_lds_limit(dev, path, monkeypatch):
    """every per-sample loop of the attention kernels strides by the wave: lengths around 16, 64, 128 and the LDS limit 2048,
    all in one batch at max_len 2048"""
    monkeypatch.setattr(dense, "ROWS_GEMM_MIN_ROWS", 0)
    monkeypatch.setattr(dense, "OWN_ROWS_GEMM", path == "own")
    D, hidden = (32, [64, 64]) if path == "own" else (16, [24, 8])
    _check(dev, D, hidden, LENGTHS, DIN_JAGGED_MAX_LEN, own=path == "own", seed=1)


def test_max_len_limit(dev):
    """tzr_din_attn_fwd / _bwd take max_len up to DA_MAXLEN = 2048 (a sample's scores in LDS) and refuse 2049; forward_jagged
    refuses it before any launch"""
    L = _lib.lib()
    D, H, B = 8, 4, 2
    off = _offsets([3, 0], dev)
    h, w3 = torch.randn(3, H).to(dev), torch.randn(H).to(dev)
    kv, gout = torch.randn(3, D).to(dev), torch.randn(B, D).to(dev)
    out, p = torch.empty(B, D).to(dev), torch.empty(3).to(dev)
    ds, dkv = torch.empty(3).to(dev), torch.empty(3, D).to(dev)
    s = _lib.stream_ptr(dev)
    for max_len, rc in ((DIN_JAGGED_MAX_LEN, 0), (DIN_JAGGED_MAX_LEN + 1, UNSUPPORTED)):
        assert L.tzr_din_attn_fwd(_lib.ptr(h), H, H, _lib.ptr(w3), None, _lib.ptr(kv), D, D, _lib.ptr(off), B, max_len, _lib.ptr(out), D,
                                  _lib.ptr(p), s) == rc
        assert L.tzr_din_attn_bwd(_lib.ptr(gout), D, _lib.ptr(p), _lib.ptr(kv), D, D, _lib.ptr(off), B, max_len, _lib.ptr(ds), _lib.ptr(dkv),
                                  D, s) == rc
    if dev.type == "cuda":
        torch.cuda.synchronize()
    enc = DINEncoder(D, D, "seq", {"hidden_units": [8, 4]}).to(dev)
    with pytest.raises(ValueError, match="max_len 2049"):
        enc.forward_jagged(gout, kv, off, DIN_JAGGED_MAX_LEN + 1)
    # max_seq_length caps it: the same call is fine
    enc = DINEncoder(D, D, "seq", {"hidden_units": [8, 4]}, max_seq_length=100).to(dev)
    assert tuple(enc.forward_jagged(gout, kv, off, DIN_JAGGED_MAX_LEN + 1).shape) == (B, D)


@pytest.mark.parametrize("max_len,msl", [(100, 0), (100, 70), (300, 33)])
@pytest.mark.parametrize("path", ["library", "own"])
def test_truncation_past_a_wave_of_rows(dev, max_len, msl, path, monkeypatch):
    """a sample of 300 rows cut at max_len 100 (200 rows behind the cut: the p / ds / dk zeroing loops go round more than once),
    and `max_seq_length` below the padded length"""
    monkeypatch.setattr(dense, "ROWS_GEMM_MIN_ROWS", 0)
    monkeypatch.setattr(dense, "OWN_ROWS_GEMM", path == "own")
    D, hidden = (48, [128, 64]) if path == "own" else (20, [16, 12])
    lens = [300, 0, 1, 99, 100, 101, 165, 71, 69, 3]
    _check(dev, D, hidden, lens, max_len, msl=msl, own=path == "own", seed=2)


def test_empty_batches(dev):
    """every sample empty (output 0, no gradient), and B = 0"""
    got = _check(dev, 16, [16, 8], [0, 0, 0, 0, 0], 100, seed=3)
    assert bool((got[0] == 0).all()) and bool((got[1] == 0).all())
    for rb in (1, 64):
        torch.manual_seed(0)
        enc = DINEncoder(16, 16, "seq", {"hidden_units": [16, 8]}).to(dev)
        got = _product(enc, torch.zeros(0, 16).to(dev), torch.zeros(0, 16).to(dev), _offsets([], dev), torch.zeros(0, dtype=torch.int64).to(dev),
                       100, torch.zeros(0, 16).to(dev), "jagged", rb)
        assert tuple(got[0].shape) == (0, 16) and tuple(got[1].shape) == (0, 16) and tuple(got[2].shape) == (0, 16)
        assert all(bool((g_ == 0).all()) for g_ in got[3:])


# ---- widths -------------------------------------------------------------------------------------------------------------------
WIDTH_LENS = [0, 1, 5, 17, 64, 65, 130, 9]


@pytest.mark.parametrize("D", [4, 8, 12, 20, 32, 48, 64, 68, 128, 252, 256])
def test_sequence_widths(dev, D):
    """sequence rows D from 4 to 256: the weighted sum's column loop goes round twice past 64 floats, the assemble backward
    splits a wave into 64 / (D / 4) position groups (unevenly at 20, 68, 252)"""
    _check(dev, D, [16, 8], WIDTH_LENS, 200, seed=D)


@pytest.mark.parametrize("D,qd", [(20, 12), (68, 20), (256, 48), (128, 4)])
def test_query_narrower_than_the_rows(dev, D, qd):
    _check(dev, D, [16, 8], WIDTH_LENS, 200, qd=qd, seed=D + qd)


@pytest.mark.parametrize("H", [4, 12, 64, 128, 256])
@pytest.mark.parametrize("row_bucket", [1, 64])
def test_last_hidden_widths_library_path(dev, H, row_bucket, monkeypatch):
    """last attention-MLP width H: the score dot (da_row_dots) goes round twice past 64; the MLP through the GEMM library with
    its rows rounded up to `row_bucket`"""
    monkeypatch.setattr(dense, "OWN_ROWS_GEMM", False)
    _check(dev, 16, [32, H], WIDTH_LENS, 200, row_bucket=row_bucket, own=False, seed=H)


@pytest.mark.parametrize("D,hidden", [(16, [64, 64]), (32, [256, 64]), (48, [256, 64]), (64, [128, 64]), (96, [128, 64]), (128, [64, 64])])
def test_own_products_shapes(dev, D, hidden, monkeypatch):
    """the library's own tall-input products (csrc/gemm_rows.hip, the query's block of the first layer once per sample) at the
    shapes _DinTowerFn._own_products takes"""
    monkeypatch.setattr(dense, "ROWS_GEMM_MIN_ROWS", 0)
    monkeypatch.setattr(dense, "OWN_ROWS_GEMM", True)
    _check(dev, D, hidden, WIDTH_LENS, 200, own=True, seed=D + hidden[0])


# ---- encoders outside the kernels' limits stay on the padded form --------------------------------------------------------------
@pytest.mark.parametrize("D,hidden,limit", [(16, [24, 6], "last attention-MLP width 6"), (272, [16, 8], "sequence_dim 272"),
                                            (18, [16, 8], "sequence_dim 18")])
def test_encoder_outside_the_kernel_limits(dev, D, hidden, limit):
    """DINEncoder.jagged_capable() states every limit of the jagged kernels; forward_jagged refuses the rest with a ValueError
    before any launch (the last width must be a multiple of 4: tzr_din_attn_fwd; rows at most 256 wide: tzr_din_assemble_bwd)"""
    enc = DINEncoder(D, 16, "seq", {"hidden_units": hidden}).to(dev)
    assert not enc.jagged_capable()
    off = _offsets([2, 0, 3], dev)
    with pytest.raises(ValueError, match=limit):
        enc.forward_jagged(torch.randn(3, 16).to(dev), torch.randn(5, D).to(dev), off, 10)
    # the padded form evaluates it against the oracle
    lens = torch.tensor([2, 0, 3]).to(dev)
    q, v, gw = torch.randn(3, 16).to(dev), torch.randn(5, D).to(dev), torch.randn(3, D).to(dev)
    want = _reference(enc, q, v, lens, 10, gw)
    got = _product(enc, q, v, off, lens, 10, gw, "padded")
    for name, a_, w_ in zip(_names(enc), got, want):
        if name != "linear.bias":
            _close(a_.to(w_.device), w_, float(w_.abs().max()), name)


def _taobao(hidden="[256, 64]", seq_dim=16, rows=1000):
    from torcheasyrec_amd.example_configs import multi_tower_din_taobao

    txt = multi_tower_din_taobao(batch_size=16, sequence_length=100)
    txt = re.sub(r"(num_buckets|hash_bucket_size): (\d+)", lambda m: f"{m.group(1)}: {min(int(m.group(2)), rows)}", txt)
    txt = txt.replace("attn_mlp { hidden_units: [256, 64] }", f"attn_mlp {{ hidden_units: {hidden} }}")
    head, sep, tail = txt.partition("sequence_feature {")
    seq, sep2, rest = tail.partition("model_config")
    return head + sep + seq.replace("embedding_dim: 16", f"embedding_dim: {seq_dim}") + sep2 + rest


@pytest.mark.parametrize("case", ["last_width_6", "rows_288_wide"])
def test_config_outside_the_kernel_limits_trains_on_the_padded_form(dev, case):
    """multi_tower_din_taobao with attn_mlp [256, 6], or with sequence rows 3 x 96 = 288 wide: the tower is built without routing
    its group onto the jagged kernels, and a training step's forward + backward runs"""
    from test_config_plumbing import _din_batches
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.rank_model import build_rank_model

    spec = load_pipeline_spec(_taobao(hidden="[256, 6]") if case == "last_width_6" else _taobao(seq_dim=96))
    torch.manual_seed(0)
    model = build_rank_model(spec, device=dev)
    din = model.din_towers[0]
    batch = next(_din_batches(spec, 16, 16, seed=5)).to(dev)
    pred = model(batch)
    loss = sum(model.loss(pred, batch).values())
    loss.backward()
    assert din._sequence_dim == (48 if case == "last_width_6" else 288) and not din.jagged_capable()
    assert "seq" not in model.embedding_group.jagged_sequence_groups
    assert bool(torch.isfinite(loss.detach()))
    for n, p_ in din.named_parameters():
        assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), n
    assert float(din.mlp.mlp[0].weight.grad.abs().sum()) > 0


def test_config_inside_the_limits_stays_jagged(dev):
    """the same config at its own widths routes the group onto the jagged kernels (the gate is no wider than the limits)"""
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.rank_model import build_rank_model

    model = build_rank_model(load_pipeline_spec(_taobao(hidden="[256, 4]", seq_dim=64)), device=dev)  # rows 3 x 64 = 192
    assert model.din_towers[0].jagged_capable() and model.embedding_group.jagged_sequence_groups == {"seq"}


# ---- grid caps ----------------------------------------------------------------------------------------------------------------
def test_more_samples_than_the_attention_grid(dev):
    """B = 16 500 > 4 096 workgroups x 4 waves: the attention kernels' sample loops and the assemble backward go round again.
    D = 64 everywhere; D = 8 on the GPU only: at D / 4 < 16 the weighted sum's column loop (which shuffles) is skipped by some
    lanes, and the lane emulator's barriers do not tell one shuffle from another, so those lanes run ahead into the wave's next
    sample there -- a wave on the hardware runs its lanes in lockstep."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 4, size=16500)
    lens[[0, 16383, 16384, 16499]] = [0, 3, 2, 1]
    for D in (64, 8) if dev.type == "cuda" else (64,):
        _check(dev, D, [16, 8], lens, 8, seed=11 + D, padded=False)


def test_more_elements_than_the_assemble_grid(dev):
    """N D / 4 > 16 384 workgroups x 256 lanes = 4 194 304 float4s (D = 256, 66 560 rows): the assemble kernels' element loops go
    round again"""
    lens = np.full(520, 128)
    lens[[0, 519]] = [0, 256]
    assert int(lens.sum()) * 256 // 4 > 16384 * 256
    _check(dev, 256, [8, 4], lens, 128, seed=12, padded=False)


# ---- full size on the GPU -----------------------------------------------------------------------------------------------------
def _native():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    _lib.use_native()
    assert _lib.backend().startswith("hip")
    return torch.device("cuda", 0)


@pytest.mark.gpu
def test_config4_full_size():
    """config 4's tower at its size: B = 8 192, histories of 0..100 clicks (some longer, cut at 100), rows of 3 x 16 = 48,
    attention MLP [256, 64] on the own products; against the float64 reference on the device"""
    dev = _native()
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 101, size=8192)
    lens[:3] = [0, 1, 100]
    lens[rng.choice(np.arange(3, 8192), 40, replace=False)] = rng.integers(101, 400, size=40)
    calls0 = _DinTowerFn.own_calls
    _check(dev, 48, [256, 64], lens, 100, own=True, seed=4)
    assert _DinTowerFn.own_calls > calls0


@pytest.mark.gpu
def test_jagged_ops_past_their_grid_cap():
    """jagged_to_padded_dense (B max_len D / 4 = 9.8 M float4s) and segment_reduce (S D / 4 = 4.8 M) past the 16 384-workgroup cap,
    forward and backward: the copies bit for bit, the sums against float64"""
    dev = _native()
    rng = np.random.default_rng(5)
    B, L, D = 8192, 100, 48
    lens = torch.from_numpy(rng.integers(0, 130, size=B))
    lens[:2] = torch.tensor([0, 129])
    v = torch.randn(int(lens.sum()), D)
    vd = v.to(dev).requires_grad_(True)
    lt = lens.to(dev)
    out = jagged_to_padded_dense(vd, _offsets(lens.numpy(), dev), L, -1.5)
    want = _pad(v.to(dev), lt, L) + (torch.arange(L, device=dev).unsqueeze(0) >= lt.unsqueeze(1)).unsqueeze(2) * -1.5
    assert torch.equal(out.detach(), want)
    g = torch.randn(B, L, D).to(dev)
    out.backward(g)
    vr = v.to(dev).requires_grad_(True)
    _pad(vr, lt, L).backward(g)
    assert torch.equal(vd.grad, vr.grad)
    S = 400_000
    seg = torch.from_numpy(rng.integers(0, 5, size=S))
    seg[:3] = torch.tensor([0, 4, 0])
    ids = torch.repeat_interleave(torch.arange(S), seg).to(dev)  # segment of every row
    x = torch.randn(int(seg.sum()), D).to(dev)
    go = torch.randn(S, D).to(dev)
    for pooling in ("sum", "mean"):
        xd = x.clone().requires_grad_(True)
        got = segment_reduce(xd, seg.to(dev), pooling)
        # float64: the rows' sum per segment (empty: 0), times 1 / length for the mean; the gradient of a row is its segment's
        # output gradient times the same factor.  A fp32 sum of <= 4 rows: <= 3 roundings of the sum of |rows|, the
        # factor 1 / length in fp32 and the product: 2 more (eps32 = 2^-24 = 6e-8 each).
        scale = (1.0 / seg.clamp_min(1).double() if pooling == "mean" else torch.ones(S, dtype=torch.float64)).to(dev).unsqueeze(1)
        want = torch.zeros(S, D, dtype=torch.float64, device=dev).index_add_(0, ids, x.double()) * scale
        mag = torch.zeros(S, D, dtype=torch.float64, device=dev).index_add_(0, ids, x.double().abs()) * scale
        assert bool(((got.detach().double() - want).abs() <= 5 * 6e-8 * mag).all()), pooling
        got.backward(go)
        want_g = (go.double() * scale)[ids]
        assert bool(((xd.grad.double() - want_g).abs() <= 2 * 6e-8 * want_g.abs()).all()), pooling  # (g * fl(1 / length): two roundings)
