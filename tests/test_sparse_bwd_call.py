"""sparse_bwd.SparseBackward: one described problem through every launcher that takes it.  ctypes checks no argument order, so a
swapped pair of integers in a launcher is a wrong update, not an error: each route here must reproduce a numpy scatter-add
exactly (SGD, lr 0.5, small-integer gradients and half-integer weights: every sum and product is exact in any order)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.embedding import _CellsGeo  # noqa: E402
from torcheasyrec_amd.sparse_bwd import SparseBackward, grad_dsts  # noqa: E402

D, LR = 16, 0.5


def _tables(rows, rng, dev):
    """(host TzrTable[], weights on `dev`, their numpy copies): fp32 tables of dim 16, key t -> table t"""
    ws = [torch.from_numpy(rng.integers(-8, 9, size=(r, D)).astype(np.float32) / 2).to(dev) for r in rows]
    ht = np.zeros(len(rows), dtype=_lib.TABLE_DT)
    for t, (r, w) in enumerate(zip(rows, ws)):
        ht[t]["w"], ht[t]["rows"], ht[t]["dim"], ht[t]["w_stride"], ht[t]["w_dtype"] = w.data_ptr(), r, D, D, _lib.DT_F32
        ht[t]["first_order"], ht[t]["n_feats"] = t, 1
    return ht, ws, [w.cpu().numpy().copy() for w in ws]


def _sgd(dev):
    lr = torch.full((1,), LR, dtype=torch.float32, device=dev)
    return lr, _lib.TzrSparseOptim(kind=_lib.OPT_SGD, weight_decay_mode=_lib.WD_NONE, d_lr=_lib.ptr(lr), eps=1e-8)


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def test_per_id_gradients_through_plan_apply_and_direct(dev):
    """grad_mode 1, offsets = key_start: two keys onto two tables (10 and 3 rows), B = 1, segments of 5 and 2 ids with repeats"""
    L = _lib.lib()
    rows, ids, key_start = [10, 3], np.array([3, 7, 3, 0, 7, 2, 2], dtype=np.int64), np.array([0, 5, 7], dtype=np.int64)
    hf = np.zeros(2, dtype=_lib.FEATURE_DT)
    hf["dst"] = -1
    hf["table"], hf["key"], hf["order"] = [0, 1], [0, 1], [0, 1]
    g = np.random.default_rng(1).integers(-3, 4, size=(7, D)).astype(np.float32)
    try:
        for route in ("plan+apply", "direct"):
            ht, ws, want = _tables(rows, np.random.default_rng(0), dev)
            for k in range(2):
                np.subtract.at(want[k], ids[key_start[k]:key_start[k + 1]], LR * g[key_start[k]:key_start[k + 1]])
            gd = torch.from_numpy(g).to(dev)
            lr, opt = _sgd(dev)
            p = SparseBackward(dev, _lib.upload_struct(ht, dev), _lib.upload_struct(hf, dev), 2, 2, 2, 10, D, torch.from_numpy(ids).to(dev),
                               torch.from_numpy(key_start).to(dev), None, 7, 7, 1, grad_mode=1)
            if route == "direct":
                assert L.tzr_tune(b"bwd_direct", 1) == 0 and p.direct_supported()
                p.direct(_lib.zeroed_workspace(p.direct_bytes(), dev), grad_dsts([gd]), opt)
            else:
                buf = _lib.workspace(p.plan_bytes(), dev)
                p.plan(buf)
                p.apply(buf, grad_dsts([gd]), opt)
            _sync(dev)
            for k in range(2):
                assert torch.equal(ws[k].cpu(), torch.from_numpy(want[k])), (route, k)
    finally:
        L.tzr_tune(b"bwd_direct", 0)


def test_pooled_gradients_through_plan_apply_cells_and_direct(dev):
    """grad_mode 0, offsets None (one id per bag): one key, one table of 10 rows, B = 4 with a repeated id"""
    L = _lib.lib()
    B, ids = 4, np.array([1, 5, 1, 9], dtype=np.int64)
    hf = np.zeros(1, dtype=_lib.FEATURE_DT)
    hf["dst"] = -1
    hf[0]["table"], hf[0]["key"], hf[0]["order"], hf[0]["n_dst"], hf[0]["dst"][0], hf[0]["col"][0] = 0, 0, 0, 1, 0, 0
    g = np.random.default_rng(2).integers(-3, 4, size=(B, D)).astype(np.float32)
    try:
        for route in ("plan+apply", "cells", "direct"):
            ht, ws, want = _tables([10], np.random.default_rng(0), dev)
            np.subtract.at(want[0], ids, LR * g)
            gd = torch.from_numpy(g).to(dev)
            lr, opt = _sgd(dev)
            p = SparseBackward(dev, _lib.upload_struct(ht, dev), _lib.upload_struct(hf, dev), 1, 1, 1, 10, D, torch.from_numpy(ids).to(dev),
                               None, None, B, B, B)
            if route == "direct":
                assert L.tzr_tune(b"bwd_direct", 1) == 0 and p.direct_supported()
                p.direct(_lib.zeroed_workspace(p.direct_bytes(), dev), grad_dsts([gd]), opt)
            elif route == "cells":
                info = (C.c_int64 * 8)()
                assert L.tzr_bwd_cells_geometry(ht.ctypes.data, 1, hf.ctypes.data, 1, B, D, None, 0, info) == _lib.TZR_OK
                img = np.zeros(int(info[0]), dtype=np.uint8)
                assert L.tzr_bwd_cells_geometry(ht.ctypes.data, 1, hf.ctypes.data, 1, B, D, img.ctypes.data, img.nbytes, info) == _lib.TZR_OK
                geo = _CellsGeo(img, info, dev)
                buf = _lib.workspace(p.plan_bytes(), dev)
                p.cells_plan(geo, buf)
                p.cells_apply(geo, buf, grad_dsts([gd]), opt)
            else:
                buf = _lib.workspace(p.plan_bytes(), dev)
                p.plan(buf)
                p.apply(buf, grad_dsts([gd]), opt)
            _sync(dev)
            assert torch.equal(ws[0].cpu(), torch.from_numpy(want[0])), route
    finally:
        L.tzr_tune(b"bwd_direct", 0)


def test_every_count_differs_a_shared_key_and_per_sample_weights(dev):
    """The two cases above leave counts equal (tables = lookups = keys; ids = positions).  Here none are: 2 tables, 3 lookups, 4 keys,
    B = 3, 12 ids, 9 positions -- key 2 is read through BOTH tables, key 0 through the second, keys 1 and 3 through none -- so a
    launcher that swaps tables with lookups or keys, or the batch size with a count of ids, updates other rows.  Once without and once with per-sample weights
    (the cells plan takes none); the one-launch form also with `hot_rows`, which must change nothing here."""
    L = _lib.lib()
    B, K = 3, 4
    ids = np.array([2, 0, 2, 1, 1, 1, 1, 2, 1, 0, 0, 0], dtype=np.int64)  # key-major [K, B]; every id < 3, the smaller table
    lookups = [(2, 0, 0), (2, 1, 16), (0, 1, 32)]  # (key, table, gradient column), in table-major order
    hf = np.zeros(3, dtype=_lib.FEATURE_DT)
    hf["dst"] = -1
    for o, (k, t, col) in enumerate(lookups):
        hf[o]["table"], hf[o]["key"], hf[o]["order"], hf[o]["n_dst"], hf[o]["dst"][0], hf[o]["col"][0] = t, k, o, 1, 0, col
    g = np.random.default_rng(3).integers(-3, 4, size=(B, 48)).astype(np.float32)
    wts = np.random.default_rng(4).integers(1, 5, size=K * B).astype(np.float32) / 2
    try:
        for weighted in (False, True):
            for route in ("plan+apply", "direct", "direct+hot_rows") + (() if weighted else ("cells",)):
                ht, ws, want = _tables([10, 3], np.random.default_rng(0), dev)
                ht[1]["first_order"], ht[1]["n_feats"] = 1, 2
                for k, t, col in lookups:
                    for b in range(B):
                        i = k * B + b
                        want[t][ids[i]] -= LR * (wts[i] if weighted else 1.0) * g[b, col:col + D]
                gd = torch.from_numpy(g).to(dev)
                lr, opt = _sgd(dev)
                p = SparseBackward(dev, _lib.upload_struct(ht, dev), _lib.upload_struct(hf, dev), 2, 3, K, 10, D, torch.from_numpy(ids).to(dev),
                                   None, torch.from_numpy(wts).to(dev) if weighted else None, K * B, 3 * B, B)
                if route.startswith("direct"):
                    assert L.tzr_tune(b"bwd_direct", 1) == 0 and p.direct_supported()
                    p.direct(_lib.zeroed_workspace(p.direct_bytes(), dev), grad_dsts([gd]), opt, hot_rows=route.endswith("hot_rows"))
                elif route == "cells":
                    info = (C.c_int64 * 8)()
                    assert L.tzr_bwd_cells_geometry(ht.ctypes.data, 2, hf.ctypes.data, 3, B, D, None, 0, info) == _lib.TZR_OK
                    img = np.zeros(int(info[0]), dtype=np.uint8)
                    assert L.tzr_bwd_cells_geometry(ht.ctypes.data, 2, hf.ctypes.data, 3, B, D, img.ctypes.data, img.nbytes, info) == _lib.TZR_OK
                    geo = _CellsGeo(img, info, dev)
                    buf = _lib.workspace(p.plan_bytes(), dev)
                    p.cells_plan(geo, buf)
                    p.cells_apply(geo, buf, grad_dsts([gd]), opt)
                else:
                    buf = _lib.workspace(p.plan_bytes(), dev)
                    p.plan(buf)
                    p.apply(buf, grad_dsts([gd]), opt)
                _sync(dev)
                for t in range(2):
                    assert torch.equal(ws[t].cpu(), torch.from_numpy(want[t])), (weighted, route, t)
    finally:
        L.tzr_tune(b"bwd_direct", 0)
