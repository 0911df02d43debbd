"""Linear layers over a tall input on the matrix cores (csrc/gemm_rows.hip: tzr_linear_rows, tzr_linear_rows_wgrad) against
torch's fp32 products -- the attention MLP of DIN on the jagged positions (/root/reference/tzrec/modules/sequence.py:101-128).
Tolerance: exact-fp32 MFMA sums in another order than torch's GEMM: <= 2e-6 of the row's / column's absolute-value product
(|x| @ |W|), the bound of a reordered fp32 sum of that length."""
import numpy as np
import pytest
import torch

from torcheasyrec_amd import _lib


def _close(got, want, scale, tol=4e-6):
    err = (got - want).abs()
    assert bool((err <= tol * scale + 1e-7).all()), float((err / (scale + 1e-30)).max())


# (K, H) pairs out of the kernel's list; N values: not a multiple of the tile, fewer rows than one tile, many turns per workgroup
@pytest.mark.parametrize("K,H", [(96, 256), (144, 256), (256, 64), (48, 64), (64, 128), (256, 256), (192, 256)])
@pytest.mark.parametrize("N,cap", [(1000, 0), (7, 0), (333, 3)])
@pytest.mark.parametrize("mode", ["bias_relu", "rowvec", "plain"])
def test_linear_rows_forward_matches_torch(dev, K, H, N, cap, mode):
    from torcheasyrec_amd.dense import linear_rows, linear_rows_supported

    g = torch.Generator().manual_seed(K * 1000 + H + N)
    x = torch.randn(N, K + 8, generator=g)[:, :K + 8]
    W = torch.randn(H, K, generator=g) / K ** 0.5
    b = torch.randn(H, generator=g)
    R = 5
    rv = torch.randn(R, H, generator=g)
    idx = torch.randint(0, R, (N,), generator=g, dtype=torch.int32)
    xd = x.to(dev)
    assert linear_rows_supported(xd, K, H)
    if mode == "rowvec" and not _lib.lib().tzr_linear_rows_supported(K, H) & 2:
        L = _lib.lib()  # (shapes whose row-vector form is not built refuse it)
        assert L.tzr_linear_rows(_lib.ptr(xd), xd.stride(0), _lib.ptr(W.to(dev)), K, 1, None, _lib.ptr(rv.to(dev)), H, _lib.ptr(idx.to(dev)), 1, N, K,
                                 H, _lib.ptr(torch.empty(N, H).to(dev)), H, _lib.stream_ptr(dev)) == -4
        return
    if cap:
        _lib.lib().tzr_tune(b"gemm_rows_wg", cap)
    try:
        if mode == "bias_relu":
            got = linear_rows(xd, W.to(dev), b.to(dev), relu=True, K=K)
            want = torch.relu(x[:, :K].double() @ W.double().t() + b.double())
        elif mode == "rowvec":
            got = linear_rows(xd, W.to(dev), None, relu=True, rowvec=rv.to(dev), row_index=idx.to(dev), K=K)
            want = torch.relu(x[:, :K].double() @ W.double().t() + rv.double()[idx.long()])
        else:
            got = linear_rows(xd, W.to(dev), K=K)
            want = x[:, :K].double() @ W.double().t()
        again = linear_rows(xd, W.to(dev), b.to(dev), relu=True, K=K) if mode == "bias_relu" else None
    finally:
        _lib.lib().tzr_tune(b"gemm_rows_wg", 0)
    scale = x[:, :K].abs().double() @ W.abs().double().t() + 1.0
    _close(got.cpu().double(), want, scale)
    if again is not None:
        assert torch.equal(again.cpu(), got.cpu())


@pytest.mark.parametrize("K,H", [(256, 96), (256, 48), (64, 144), (128, 192), (256, 144), (256, 192)])
@pytest.mark.parametrize("N", [500, 16])
def test_linear_rows_input_gradient_matches_torch(dev, K, H, N):
    """g [N, K] @ weight [K, H] (the weight of a layer K <- H as nn.Linear stores it: no transpose, no copy)"""
    from torcheasyrec_amd.dense import linear_rows, linear_rows_supported

    gen = torch.Generator().manual_seed(K + 7 * H + N)
    g = torch.randn(N, K, generator=gen)
    W = torch.randn(K, H, generator=gen) / K ** 0.5
    assert linear_rows_supported(g.to(dev), K, H)
    got = linear_rows(g.to(dev), W.to(dev), out_major=False)
    want = g.double() @ W.double()
    _close(got.cpu().double(), want, g.abs().double() @ W.abs().double() + 1.0)


@pytest.mark.parametrize("H,K", [(256, 96), (256, 144), (64, 256), (256, 48), (128, 128), (64, 48)])
@pytest.mark.parametrize("N,cap", [(900, 0), (5, 0), (700, 2)])
def test_linear_rows_weight_gradient_matches_torch(dev, H, K, N, cap):
    from torcheasyrec_amd.dense import linear_rows_wgrad, linear_rows_wgrad_supported

    gen = torch.Generator().manual_seed(H + 3 * K + N)
    g = torch.randn(N, H, generator=gen)
    x = torch.randn(N, K + 4, generator=gen)
    assert linear_rows_wgrad_supported(g.to(dev), x.to(dev), K)
    if cap:
        _lib.lib().tzr_tune(b"gemm_rows_wg", cap)
    try:
        got = linear_rows_wgrad(g.to(dev), x.to(dev), K)
        again = linear_rows_wgrad(g.to(dev), x.to(dev), K)
    finally:
        _lib.lib().tzr_tune(b"gemm_rows_wg", 0)
    want = g.double().t() @ x[:, :K].double()
    _close(got.cpu().double(), want, g.abs().double().t() @ x[:, :K].abs().double() + 1.0)
    assert torch.equal(again.cpu(), got.cpu())  # no float atomics: bit-reproducible


def test_unsupported_shapes_are_refused(dev):
    from torcheasyrec_amd.dense import linear_rows_supported, linear_rows_wgrad_supported

    x = torch.randn(64, 100).to(dev)
    assert not linear_rows_supported(x, 100, 64)
    assert not linear_rows_supported(x, 96, 80)
    assert not linear_rows_wgrad_supported(torch.randn(64, 80).to(dev), x, 96)
    L = _lib.lib()
    assert L.tzr_linear_rows(_lib.ptr(x), 100, _lib.ptr(x), 100, 1, None, None, 0, None, 0, 64, 100, 64, _lib.ptr(x), 100, None) == -4  # TZR_ERR_UNSUPPORTED


# ---- every built shape, every tile tail, every argument of the C ABI ----------------------------------------------------
# The kernels are tables of template instantiations (gemm_rows.hip: GR_ROWS_CONFIGS, kTn).  The shape lists below are ASKED of
# the loaded library, not copied from it; only the widths the parametrised tests are grouped by are written down here, and
# test_shape_tables_are_complete holds them against the library's answer.
_FWD_HS = (16, 32, 48, 64, 96, 128, 144, 192, 256)  # output widths H of the forward table
_WGRAD_HS = (64, 128, 256)                           # heights H of the weight-gradient table
_M = 80                                              # rows of a forward case: five 16-row tiles, two and a half 32-row turns
_TAIL_NS = (1, 15, 16, 17, 31, 32, 33, 47, 64, 65, 70)  # last turns of 1 / 15 / 16 / 17 / 31 / 32 rows behind 0 .. 4 full tiles
_WGRAD_NS = (1, 15, 16, 17, 129)
_UNSUPPORTED, _WORKSPACE = -4, -3


def _fwd_shapes():
    L = _lib.lib()
    return [(K, H, L.tzr_linear_rows_supported(K, H)) for K in range(16, 257, 16) for H in range(16, 257, 16) if L.tzr_linear_rows_supported(K, H)]


def _wgrad_shapes():
    L = _lib.lib()
    return [(H, K) for H in range(16, 257, 16) for K in range(16, 257, 16) if L.tzr_linear_rows_wgrad_supported(H, K)]


def _note(bad, tag, got, want, scale):
    """`_close`, collected: one failing shape does not hide the others"""
    try:
        _close(got, want, scale)
    except AssertionError as e:
        bad.append((tag, "relative to |x| @ |W| + 1: " + str(e)))


_fwd_cases, _wgrad_cases = {}, {}


class _Case:
    pass


def _fwd_case(K, H):
    """inputs of one forward shape and their float64 results, made once and never written again.  Precondition of every tolerance
    test: torch's own fp32 product of the same inputs on the CPU is inside the bound -- a miss indicts the kernel, not the bound."""
    if (K, H) not in _fwd_cases:
        c = _Case()
        g = torch.Generator().manual_seed(K * 1000 + H)
        c.x = torch.randn(_M, K + 8, generator=g)  # in_stride > K
        c.W = torch.randn(H, K, generator=g) / K ** 0.5
        c.b = torch.randn(H, generator=g)
        c.rv = torch.randn(5, H, generator=g)
        c.idx = torch.randint(0, 5, (_M,), generator=g, dtype=torch.int32)
        lin = c.x[:, :K].double() @ c.W.double().t()
        add = c.rv.double()[c.idx.long()]
        c.want = {"plain": lin, "bias_relu": torch.relu(lin + c.b.double()), "rowvec_relu": torch.relu(lin + add),
                  "bias_rowvec_relu": torch.relu(lin + c.b.double() + add)}
        c.scale = c.x[:, :K].abs().double() @ c.W.abs().double().t() + 1.0
        l32 = c.x[:, :K] @ c.W.t()
        for mode, own in (("plain", l32), ("bias_relu", torch.relu(l32 + c.b)), ("rowvec_relu", torch.relu(l32 + c.rv[c.idx.long()])),
                          ("bias_rowvec_relu", torch.relu(l32 + c.b + c.rv[c.idx.long()]))):
            _close(own.double(), c.want[mode], c.scale)
        _fwd_cases[K, H] = c
    return _fwd_cases[K, H]


def _wgrad_case(H, K, N):
    if (H, K, N) not in _wgrad_cases:
        c = _Case()
        gen = torch.Generator().manual_seed(H + 3 * K + N)
        c.g = torch.randn(N, H, generator=gen)
        c.x = torch.randn(N, K + 4, generator=gen)  # x_stride > K
        c.want = c.g.double().t() @ c.x[:, :K].double()
        c.scale = c.g.abs().double().t() @ c.x[:, :K].abs().double() + 1.0
        _close((c.g.t() @ c.x[:, :K]).double(), c.want, c.scale)  # (the precondition, as in _fwd_case)
        _wgrad_cases[H, K, N] = c
    return _wgrad_cases[H, K, N]


def _rows_abi(x, N, K, H, w, out_major, bias, rv, idx, relu, out):
    """tzr_linear_rows itself: `out` may be a view into a larger buffer, `x` / `idx` may be longer than N"""
    return _lib.lib().tzr_linear_rows(_lib.ptr(x), x.stride(0), _lib.ptr(w), w.stride(0), 1 if out_major else 0, _lib.ptr(bias), _lib.ptr(rv),
                                      rv.stride(0) if rv is not None else 0, _lib.ptr(idx), 1 if relu else 0, N, K, H, _lib.ptr(out), out.stride(0),
                                      _lib.stream_ptr(x.device))


def _wgrad_abi(g, x, K, dw, accumulate, short=0):
    """tzr_linear_rows_wgrad itself, with exactly the bytes it asks for (its _workspace answer less the 256 bytes of alignment
    slack every *_workspace of this library includes) less `short`"""
    L = _lib.lib()
    N, H = g.shape
    need = L.tzr_linear_rows_wgrad_workspace(N, H, K)
    ws = _lib.workspace(need, g.device)
    return L.tzr_linear_rows_wgrad(_lib.ptr(g), g.stride(0), _lib.ptr(x), x.stride(0), N, H, K, _lib.ptr(dw), dw.stride(0), accumulate, _lib.ptr(ws),
                                   need - 256 - short, _lib.stream_ptr(g.device))


def test_shape_tables_are_complete(dev):
    """a dropped row of either table is noticed: 45 forward shapes, 25 weight gradients; 27 forward shapes are 64, 128 or 256 wide
    and 24 of those are built with the row-vector form too (never 144 -> 256, 192 -> 64, 192 -> 256: the existing test above has
    two of them refuse it)"""
    fwd, wg = _fwd_shapes(), _wgrad_shapes()
    assert len(fwd) == 45 and all(f in (1, 3) for _, _, f in fwd)
    assert sum(1 for _, H, _ in fwd if H in (64, 128, 256)) == 27
    assert sum(1 for _, _, f in fwd if f & 2) == 24 and all(H in (64, 128, 256) for _, H, f in fwd if f & 2)
    assert len(wg) == 25
    assert {H for _, H, _ in fwd} == set(_FWD_HS) and {H for H, _ in wg} == set(_WGRAD_HS)  # (what the tests below are grouped by)
    assert {K for K, _, _ in fwd} >= {16, 32}  # operand prefetch depth K / 16 = 1 and 2


def _forward_misses(dev, K, H, flags):
    """one shape, 80 rows, both weight layouts x {plain, bias + ReLU, row vector + ReLU} against float64"""
    from torcheasyrec_amd.dense import linear_rows

    c, bad = _fwd_case(K, H), []
    xd, bd, rvd, idxd = c.x.to(dev), c.b.to(dev), c.rv.to(dev), c.idx.to(dev)
    outs = {}
    for out_major in (True, False):
        wd = (c.W if out_major else c.W.t().contiguous()).to(dev)
        got = {"plain": linear_rows(xd, wd, out_major=out_major, K=K), "bias_relu": linear_rows(xd, wd, bd, relu=True, out_major=out_major, K=K)}
        if flags & 2:
            got["rowvec_relu"] = linear_rows(xd, wd, None, relu=True, out_major=out_major, rowvec=rvd, row_index=idxd, K=K)
        elif _rows_abi(xd, _M, K, H, wd, out_major, None, rvd, idxd, True, torch.empty(_M, H).to(dev)) != _UNSUPPORTED:
            bad.append(((K, H, out_major), "a row vector was not refused"))
        for mode, o in got.items():
            _note(bad, (K, H, out_major, mode), o.cpu().double(), c.want[mode], c.scale)
        outs[out_major] = got
    for mode in outs[True]:  # (both layouts fill the same weight registers: operand A of step s is W(k(s, q), .) either way)
        if not torch.equal(outs[True][mode].cpu(), outs[False][mode].cpu()):
            bad.append(((K, H, mode), "the two weight layouts differ"))
    return bad


def _tail_misses(dev, K, H, flags, ns, caps=(0, 1, 2)):
    """an output row depends on its own input row only and its sum order is fixed: the first N rows of the 80-row result, bit for
    bit, whatever N leaves in the last turn and however many workgroups walk the turns (cap 1: one workgroup, every turn, both LDS
    buffers; cap 2: with an odd turn count the two workgroups walk different numbers of turns).  Bias + ReLU, and the gathered row
    vector wherever it is built (its indices are staged with the same clamp as the rows)."""
    from torcheasyrec_amd.dense import linear_rows

    c, bad = _fwd_case(K, H), []
    xd, bd, idxd = c.x.to(dev), c.b.to(dev), c.idx.to(dev)
    rvd = c.rv.to(dev) if flags & 2 else None
    wds = {True: c.W.to(dev), False: c.W.t().contiguous().to(dev)}

    def run(n, out_major):
        return linear_rows(xd[:n], wds[out_major], bd, relu=True, out_major=out_major, rowvec=rvd, row_index=idxd[:n] if flags & 2 else None, K=K).cpu()

    base = run(_M, True)
    _note(bad, (K, H, "80 rows"), base.double(), c.want["bias_rowvec_relu" if flags & 2 else "bias_relu"], c.scale)
    try:
        for cap in caps:
            _lib.lib().tzr_tune(b"gemm_rows_wg", cap)
            for n in tuple(ns) + ((_M,) if cap else ()):
                if not torch.equal(run(n, cap != 1), base[:n]):
                    bad.append((K, H, n, cap))
    finally:
        _lib.lib().tzr_tune(b"gemm_rows_wg", 0)
    return bad


def _wgrad_misses(dev, H, K, ns):
    from torcheasyrec_amd.dense import linear_rows_wgrad

    bad = []
    for N in ns:
        c = _wgrad_case(H, K, N)
        gd, xd = c.g.to(dev), c.x.to(dev)
        got = linear_rows_wgrad(gd, xd, K).cpu()
        _note(bad, (H, K, N), got.double(), c.want, c.scale)
        if not torch.equal(linear_rows_wgrad(gd, xd, K).cpu(), got):
            bad.append(((H, K, N), "a second call differs"))
    return bad


@pytest.mark.parametrize("H", _FWD_HS)
def test_every_forward_shape_matches_float64(dev, H):
    shapes = [s for s in _fwd_shapes() if s[1] == H]
    assert shapes
    bad = [m for K, _, flags in shapes for m in _forward_misses(dev, K, H, flags)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("H", _FWD_HS)
def test_forward_tails_are_bit_exact(dev, H):
    """(all N in 1 .. 70: test_every_shape_and_row_count_on_the_emulator)"""
    shapes = [s for s in _fwd_shapes() if s[1] == H]
    assert shapes
    bad = [m for K, _, flags in shapes for m in _tail_misses(dev, K, H, flags, _TAIL_NS)]
    assert not bad, bad[:10]


# one shape per (WAVES, TT) class of the table, HB = 3, and the two shortest contractions (one and two operand reads per tile)
_GUARD_SHAPES = [(64, 16), (128, 32), (64, 48), (128, 96), (128, 144), (256, 144), (48, 64), (96, 128), (256, 256), (16, 64), (32, 128), (192, 256)]


@pytest.mark.parametrize("K,H", _GUARD_SHAPES)
def test_forward_touches_nothing_outside_its_rows(dev, K, H):
    """Rows beyond N are read as row N - 1 and stored to row N - 1's address, without a row test anywhere.  Output guard: d_out is
    a window of a NaN-filled buffer (out_stride = H + 12, spare rows before and behind) -- not one bit outside [0:N, 0:H] changes
    and the inside is the contiguous result.  Input guard: the input's rows >= N, its columns >= K and the row vector that the
    row_index entries behind N point at hold NaN (all inside the test's own allocations) -- no output is NaN.  The k-major weight
    comes with w_stride = H + 3, the row vector with rowvec_stride = H + 4."""
    from torcheasyrec_amd.dense import linear_rows

    flags = _lib.lib().tzr_linear_rows_supported(K, H)
    assert flags
    c = _fwd_case(K, H)
    nan = float("nan")
    bd = c.b.to(dev)
    wt = torch.full((K, H + 3), nan)
    wt[:, :H] = c.W.t()
    wds = {True: c.W.to(dev), False: wt.to(dev)[:, :H]}
    rvd = idxd = None
    if flags & 2:
        rv = torch.full((6, H + 4), nan)  # row 5: poison
        rv[:5, :H] = c.rv
        rvd = rv.to(dev)[:, :H]
    for N in (1, 17, 33):
        x = torch.full((N + 40, K + 8), nan)
        x[:N, :K] = c.x[:N, :K]
        xd = x.to(dev)
        if flags & 2:
            idx = torch.full((N + 40,), 5, dtype=torch.int32)
            idx[:N] = c.idx[:N]
            idxd = idx.to(dev)
        want = c.want["bias_rowvec_relu" if flags & 2 else "bias_relu"][:N]
        for out_major in (True, False):
            flat = linear_rows(xd[:N], wds[out_major], bd, relu=True, out_major=out_major, rowvec=rvd, row_index=idxd, K=K).cpu()
            assert not bool(torch.isnan(flat).any()), (N, out_major)
            _close(flat.double(), want, c.scale[:N])
            buf = torch.full((3 + N + 35, H + 12), nan).to(dev)
            before = buf.cpu().view(torch.int32).clone()
            assert _rows_abi(xd, N, K, H, wds[out_major], out_major, bd, rvd, idxd, True, buf[3:3 + N, 4:4 + H]) == 0
            after = buf.cpu()
            assert torch.equal(after[3:3 + N, 4:4 + H], flat), (N, out_major)
            inside = torch.zeros(after.shape, dtype=torch.bool)
            inside[3:3 + N, 4:4 + H] = True
            assert torch.equal(after.view(torch.int32)[~inside], before[~inside]), (N, out_major)


@pytest.mark.parametrize("H", _WGRAD_HS)
def test_every_weight_gradient_shape_matches_float64(dev, H):
    shapes = [s for s in _wgrad_shapes() if s[0] == H]
    assert shapes
    bad = [m for _, K in shapes for m in _wgrad_misses(dev, H, K, _WGRAD_NS)]
    assert not bad, bad[:10]


# tzr_gemm_tn_finish_kernel adds the workgroups' partial sums in 16 slices x 8 loads in flight, 128 workgroups per pass; a
# workgroup per 8 blocks of 16 rows: 2100 rows = 17 workgroups (the second load of slice 0), 16645 = 131 (the second pass)
@pytest.mark.parametrize("H,K,N", [(64, 16, 2100), (128, 32, 2100), (64, 16, 16645), (128, 32, 16645), (256, 144, 2100)])
def test_weight_gradient_partial_sums_of_many_workgroups(dev, H, K, N):
    """(256 x 144: 36 accumulator blocks, the form without the operand prefetch)"""
    assert _lib.lib().tzr_linear_rows_wgrad_workspace(N, H, K) == ((N + 15) // 16 + 7) // 8 * H * K * 4 + 256
    bad = _wgrad_misses(dev, H, K, (N,))
    assert not bad, bad


def test_weight_gradient_at_the_workgroup_limit_on_the_emulator(emu_path):
    """70 000 rows = 547 workgroups' worth, held at 512 (about a second on the emulator; the chip's step runs at this count)"""
    _lib.use_library(emu_path)
    assert _lib.lib().tzr_linear_rows_wgrad_workspace(70000, 64, 16) == 512 * 64 * 16 * 4 + 256
    bad = _wgrad_misses(torch.device("cpu"), 64, 16, (70000,))
    assert not bad, bad


@pytest.mark.parametrize("H", _WGRAD_HS)
@pytest.mark.parametrize("cap", [1, 3])
def test_weight_gradient_with_capped_workgroups(dev, H, cap):
    """40 blocks of rows (the last one partial) on 1 and on 3 workgroups instead of 5: with 3 the block counts are 14 / 13 / 13 and
    the last workgroups' prefetch runs dry a turn before the first's"""
    shapes = [s for s in _wgrad_shapes() if s[0] == H]
    assert shapes
    try:
        _lib.lib().tzr_tune(b"gemm_rows_wg", cap)
        bad = [m for _, K in shapes for m in _wgrad_misses(dev, H, K, (630,))]
    finally:
        _lib.lib().tzr_tune(b"gemm_rows_wg", 0)
    assert not bad, bad[:10]


@pytest.mark.parametrize("H", _WGRAD_HS)
def test_weight_gradient_abi_accumulate_stride_workspace(dev, H):
    """d_dw as the [1:H+1, 4:4+K] window of a random [H + 2, K + 12] buffer: accumulate = 1 leaves old + the plain result (the same
    bits: the finish kernel stores *o + s), accumulate = 0 the plain result, nothing outside the window changes; a workspace one
    byte short of what the kernel uses is refused"""
    from torcheasyrec_amd.dense import linear_rows_wgrad

    shapes = [s for s in _wgrad_shapes() if s[0] == H]
    assert shapes
    for _, K in shapes:
        c = _wgrad_case(H, K, 129)
        gd, xd = c.g.to(dev), c.x.to(dev)
        plain = linear_rows_wgrad(gd, xd, K).cpu()
        old = torch.randn(H + 2, K + 12, generator=torch.Generator().manual_seed(H + K))
        inside = torch.zeros(old.shape, dtype=torch.bool)
        inside[1:H + 1, 4:4 + K] = True
        for accumulate in (1, 0):
            buf = old.clone().to(dev)
            assert _wgrad_abi(gd, xd, K, buf[1:H + 1, 4:4 + K], accumulate) == 0
            got = buf.cpu()
            assert torch.equal(got[1:H + 1, 4:4 + K], old[1:H + 1, 4:4 + K] + plain if accumulate else plain), (H, K, accumulate)
            assert torch.equal(got[~inside], old[~inside]), (H, K, accumulate)
        buf = old.clone().to(dev)
        assert _wgrad_abi(gd, xd, K, buf[1:H + 1, 4:4 + K], 0, short=1) == _WORKSPACE
        assert torch.equal(buf.cpu(), old)


def test_every_shape_and_row_count_on_the_emulator(emu_path):
    """All 45 forward shapes x N = 1 .. 70 x workgroup caps 0 / 1 / 2 bit-exact against the 80-row result (9 630 launches), the 80
    rows in both layouts and all modes against float64; all 25 weight-gradient shapes against float64 with a second call
    bit-identical at the row counts that, with the parametrised test's 1 / 15 / 16 / 17 / 129, make every block count from 1 to 5
    both full and partial, and the two smallest at every N = 1 .. 70 (the row test of its loads is the same code in every
    instantiation, and a call costs the emulator a 1024-thread finish workgroup per 64 outputs whatever N is).  Emulator only,
    106 s there (81 s of it the 45 x 70 x 3 tails: 2.1 G multiply-adds); on the chip the parametrised tests above run the thinned N sets."""
    _lib.use_library(emu_path)  # (the `dev` fixture of the other tests selects its library itself)
    cpu = torch.device("cpu")
    bad = []
    for K, H, flags in _fwd_shapes():
        bad += _forward_misses(cpu, K, H, flags)
        bad += _tail_misses(cpu, K, H, flags, range(1, 71))
    for H, K in _wgrad_shapes():
        bad += _wgrad_misses(cpu, H, K, range(1, 71) if (H, K) in ((64, 16), (128, 32)) else (2, 31, 32, 33, 48, 63, 64, 70))
    assert not bad, (len(bad), bad[:10])
