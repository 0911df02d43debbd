"""Adadelta and RMSprop (tests/test_sparse_optim_elem.py) through the sharded collection at world 2 on gloo, kernels through
the lane emulator: row-wise, table-wise and replicated tables end where the unsharded collection ends on the global batch; a
column-wise table's shards end where an unsharded collection of its column blocks (one table per block, each read by the
same feature) ends -- both kinds are elementwise, so a shard that updates its own columns is exact."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.join(os.path.dirname(__file__), "..")
sys.path.insert(0, ROOT)

KINDS = ("adadelta", "rmsprop")


def _worker(rank, world, init_file, emu_path, kind):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.embedding import EmbeddingBagCollection, EmbeddingBagConfig, SparseOptimizerConfig
    from torcheasyrec_amd.sharding import MixedShardedEmbeddingBagCollection
    from torcheasyrec_amd.sparse import KeyedJaggedTensor

    _lib.use_library(emu_path)
    dev = torch.device("cpu")

    def seeded(t, cols=slice(None)):
        def f(w):
            g = torch.Generator().manual_seed(100 + t)
            full = (torch.rand(w.shape[0], 16, generator=g) - 0.5) * 0.2
            w.copy_(full[:, cols])
        return f

    spec = [("rw", 301, ["a"]), ("tw", 50, ["b"]), ("dp", 7, ["d"]), ("cw", 120, ["c"])]
    cfgs = [EmbeddingBagConfig(n, 16, r, f, init_fn=seeded(t)) for t, (n, r, f) in enumerate(spec)]
    opt = (SparseOptimizerConfig(kind=kind, lr=0.5, rho=0.9, eps=1e-6, weight_decay=0.01) if kind == "adadelta"
           else SparseOptimizerConfig(kind=kind, lr=0.002, alpha=0.9, eps=1e-8, weight_decay=0.01))
    groups = {"g": ["a", "b", "d", "c"]}
    sh = MixedShardedEmbeddingBagCollection(cfgs, device=dev, optimizer=opt, groups=groups, dp_max_rows=10,
                                            constraints={"cw": "column_wise", "tw": "table_wise"})
    plan = sh.sharding_plan()
    assert [plan[n]["sharding_type"] for n in ("rw", "tw", "dp", "cw")] == ["row_wise", "table_wise", "data_parallel",
                                                                            "column_wise"]
    assert plan["cw"]["shard_dim"] == 8
    # the restatement of the column-wise table: one unsharded table per column block, both read by feature c
    ref_cfgs = [EmbeddingBagConfig(n, 16, r, f, init_fn=seeded(t)) for t, (n, r, f) in enumerate(spec[:3])] + [
        EmbeddingBagConfig("cw_lo", 8, 120, ["c"], init_fn=seeded(3, slice(0, 8))),
        EmbeddingBagConfig("cw_hi", 8, 120, ["c"], init_fn=seeded(3, slice(8, 16)))]
    ref = EmbeddingBagCollection(ref_cfgs, device=dev, optimizer=opt, groups={"g": ["a", "b", "d", "c@cw_lo", "c@cw_hi"]})
    keys, rows = ["a", "b", "d", "c"], [301, 50, 7, 120]
    rng = np.random.default_rng(0)
    Bg, Bl = 40, 20
    for step in range(3):
        ids = np.stack([rng.integers(0, r, size=Bg) for r in rows]).astype(np.int64)
        ids[:, :4] = 0  # duplicates across ranks
        g = torch.randn(Bg, 64, generator=torch.Generator().manual_seed(9 + step))
        mine = KeyedJaggedTensor(keys, torch.from_numpy(ids[:, rank * Bl:(rank + 1) * Bl].reshape(-1).copy()),
                                 torch.ones(4 * Bl, dtype=torch.int32), uniform_length=1)
        full = KeyedJaggedTensor(keys, torch.from_numpy(ids.reshape(-1).copy()), torch.ones(4 * Bg, dtype=torch.int32),
                                 uniform_length=1)
        out = sh.forward_grouped(mine)["g"]
        out_ref = ref.forward_grouped(full)["g"]
        torch.testing.assert_close(out.detach(), out_ref.detach()[rank * Bl:(rank + 1) * Bl], rtol=1e-5, atol=1e-6)
        (out * g[rank * Bl:(rank + 1) * Bl]).sum().backward()
        (out_ref * g).sum().backward()
    assert sh.fused_optimizer._adam is None and ref.fused_optimizer._adam is None  # no step counter for these kinds
    w, s = sh.table_weights(), sh.table_states()
    w_ref, s_ref = ref.table_weights(), ref.table_states()
    for name in ("rw", "tw", "dp"):
        lo, n = sh.shard_of(name)
        torch.testing.assert_close(w[name].detach()[:n], w_ref[name].detach()[lo:lo + n], rtol=2e-5, atol=1e-6, msg=name)
        torch.testing.assert_close(s[name].detach()[:n], s_ref[name].detach()[lo:lo + n], rtol=2e-5, atol=1e-7, msg=name)
    for j, shard in enumerate(sh.column_shards("cw")):
        lo, n = sh.shard_of(shard)
        rn = ("cw_lo", "cw_hi")[j]
        assert s[shard].shape[1] == s_ref[rn].shape[1] == (16 if kind == "adadelta" else 8)  # the shard's own state layout (D = 8)
        torch.testing.assert_close(w[shard].detach()[:n], w_ref[rn].detach()[lo:lo + n], rtol=2e-5, atol=1e-6, msg=shard)
        torch.testing.assert_close(s[shard].detach()[:n], s_ref[rn].detach()[lo:lo + n], rtol=2e-5, atol=1e-7, msg=shard)
    fresh = torch.empty(301, 16)
    seeded(0)(fresh)
    assert not torch.equal(w_ref["rw"].detach(), fresh)  # the steps moved the tables
    assert all(float(s_ref[n].abs().sum()) > 0.0 for n in s_ref)
    dist.barrier()
    dist.destroy_process_group()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


@pytest.mark.parametrize("kind", KINDS)
def test_elem_kinds_sharded_world2(emu_path, kind):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), emu_path, kind), nprocs=2, join=True)
