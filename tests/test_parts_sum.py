"""The two fixed orders in which rows of per-workgroup partial sums are added up (csrc/parts_sum.h; documented as part of the
ABI in include/tzrec_hip.h), pinned BIT FOR BIT against an oracle that performs the documented additions in numpy float32, one
row vector at a time.  fp32 additions are IEEE-exact on both backends, so the oracle holds on the emulator and on the chip.

interleaved   sixteen chains take the rows s, s + 16, s + 32, ..., then the sixteen chain sums are added 0..15
              (tzr_relu_bwd_colsum's finish; its rows are what tzr_relu_bwd_colsum_parts leaves at the head of `ws`)
blocked       sixteen contiguous ranges of ceil(G / 16) rows, then the sixteen range sums 0..15
              (tzr_mlp2_bwd's finish, and every TZR_ADAM_SRC_ROWS source of tzr_dense_adam_fused)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from torcheasyrec_amd import _lib  # noqa: E402


def interleaved_sum(rows: np.ndarray) -> np.ndarray:
    G, N = rows.shape
    total = np.zeros(N, np.float32)
    for s in range(16):
        chain = np.zeros(N, np.float32)
        for k in range(s, G, 16):
            chain = chain + rows[k]
        total = total + chain
    return total


def blocked_sum(rows: np.ndarray) -> np.ndarray:
    G, N = rows.shape
    per = (G + 15) // 16
    total = np.zeros(N, np.float32)
    for q in range(16):
        part = np.zeros(N, np.float32)
        for g in range(q * per, min(G, (q + 1) * per)):
            part = part + rows[g]
        total = total + part
    return total


def test_the_two_oracles_differ_where_the_orders_do():
    """(the tests below would pass with the orders swapped if the two sums rounded alike on their inputs: they do not)"""
    rows = torch.randn(129, 64, generator=torch.Generator().manual_seed(0)).numpy()
    assert rows.dtype == np.float32 and interleaved_sum(rows).dtype == np.float32
    assert not np.array_equal(interleaved_sum(rows), blocked_sum(rows))
    np.testing.assert_allclose(interleaved_sum(rows), rows.astype(np.float64).sum(0), rtol=0, atol=1e-4)
    np.testing.assert_allclose(blocked_sum(rows), rows.astype(np.float64).sum(0), rtol=0, atol=1e-4)


# N = 1024: one row per sweep, four rows per workgroup -- the first, the last and the wrapped slice, the second pass of eight
# loads, the workgroup cap.  N = 68: a second column tile with four live columns (15 rows per sweep, 60 per workgroup).
# N = 4: 256 rows per sweep.
@pytest.mark.parametrize("N,B,G", [(1024, 4, 1), (1024, 60, 15), (1024, 64, 16), (1024, 68, 17), (1024, 508, 127), (1024, 512, 128),
                                   (1024, 516, 129), (1024, 4096, 1024), (68, 1000, 17), (68, 7700, 129), (4, 17 * 1024, 17)])
def test_relu_bwd_colsum_adds_its_rows_in_the_interleaved_order(dev, N, B, G):
    L = _lib.lib()
    gen = torch.Generator().manual_seed(N + B)
    gy, y = torch.randn(B, N, generator=gen).to(dev), torch.randn(B, N, generator=gen).to(dev)
    ws = _lib.workspace(L.tzr_relu_bwd_colsum_workspace(B, N), dev)
    g_parts, g_fin = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
    colsum = torch.empty(N, device=dev)
    got_G = C.c_int(0)
    _lib.check(L.tzr_relu_bwd_colsum_parts(_lib.ptr(gy), N, _lib.ptr(y), N, B, N, _lib.ptr(g_parts), N, _lib.ptr(ws), ws.numel(),
                                           C.byref(got_G), _lib.stream_ptr(dev)), "tzr_relu_bwd_colsum_parts")
    assert got_G.value == G
    rows = ws[:G * N * 4].clone().cpu().view(torch.float32).view(G, N).numpy().copy()
    _lib.check(L.tzr_relu_bwd_colsum(_lib.ptr(gy), N, _lib.ptr(y), N, B, N, _lib.ptr(g_fin), N, _lib.ptr(colsum), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr(dev)), "tzr_relu_bwd_colsum")
    assert torch.equal(g_parts.cpu(), g_fin.cpu())
    assert torch.equal(g_fin.cpu(), torch.where(y.cpu() > 0, gy.cpu(), torch.zeros(())))
    assert torch.equal(colsum.cpu(), torch.from_numpy(interleaved_sum(rows)))


@pytest.mark.parametrize("G", [1, 15, 16, 17, 129, 512])
def test_a_rows_source_of_the_fused_adam_is_added_in_the_blocked_order(dev, G):
    """a store-only call (param == 0): numel = 33 of P = 40 columns from col = 3 -- the last 16-output workgroup is partial, the
    column offset is live"""
    P, col, numel = 40, 3, 33
    rows = torch.randn(G, P, generator=torch.Generator().manual_seed(G))
    buf, grad = rows.to(dev), torch.full((numel + 2,), 7.0, device=dev)
    tab, src = (_lib.TzrAdamTensor * 1)(), (_lib.TzrAdamSource * 1)()
    tab[0].param, tab[0].grad, tab[0].numel = 0, _lib.ptr(grad), numel
    src[0].kind, src[0].G, src[0].P, src[0].col, src[0].parts = _lib.ADAM_SRC_ROWS, G, P, col, _lib.ptr(buf)
    _lib.check(_lib.lib().tzr_dense_adam_fused(tab, src, 1, None, None, 0.0, 0.9, 0.999, 1e-8, 0.0, _lib.stream_ptr(dev)),
               "tzr_dense_adam_fused")
    got = grad.cpu()
    assert torch.equal(got[:numel], torch.from_numpy(blocked_sum(rows.numpy()[:, col:col + numel])))
    assert got[numel:].tolist() == [7.0, 7.0]  # (nothing behind the tensor's last element is written)


def test_mlp2_bwd_finishes_its_rows_in_the_blocked_order(dev):
    """the separate finishing launch of tzr_mlp2_bwd == the oracle over the rows tzr_mlp2_bwd_parts leaves: the smallest
    supported widths, 17 sample tiles = 17 rows (one range of one row behind eight of two)"""
    L = _lib.lib()
    B, K0, H1, H2 = 17 * 64 - 28, 1, 1, 1
    gen = torch.Generator().manual_seed(0)
    dhb, hb, ha, x = (torch.randn(B, n, generator=gen).to(dev) for n in (H2, H2, H1, K0))
    Wb = torch.randn(H2, H1, generator=gen).to(dev)
    ws = _lib.workspace(L.tzr_mlp_workspace(), dev)
    G, P = C.c_int(0), C.c_int(0)
    args = (_lib.ptr(dhb), H2, _lib.ptr(hb), H2, _lib.ptr(ha), H1, _lib.ptr(x), K0, B, K0, H1, H2, _lib.ptr(Wb))
    _lib.check(L.tzr_mlp2_bwd_parts(*args, _lib.ptr(ws), ws.numel(), C.byref(G), C.byref(P), _lib.stream_ptr(dev)), "tzr_mlp2_bwd_parts")
    assert (G.value, P.value) == (17, H2 * H1 + H2 + H1 * K0 + H1)
    want = blocked_sum(ws[:G.value * P.value * 4].clone().cpu().view(torch.float32).view(G.value, P.value).numpy().copy())
    dWb, dbb, dWa, dba = (torch.empty(n, device=dev) for n in (H2 * H1, H2, H1 * K0, H1))
    _lib.check(L.tzr_mlp2_bwd(*args, _lib.ptr(dWa), _lib.ptr(dba), _lib.ptr(dWb), _lib.ptr(dbb), _lib.ptr(ws), ws.numel(),
                              _lib.stream_ptr(dev)), "tzr_mlp2_bwd")
    assert torch.equal(torch.cat([dWb, dbb, dWa, dba]).cpu(), torch.from_numpy(want))
    assert bool(want.any())
