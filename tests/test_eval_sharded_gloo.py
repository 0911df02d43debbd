"""The evaluation metrics over two gloo ranks (CPU, the lane emulator): every rank updates with its half of each batch, and
`compute()` -- the histogram and the NE sums all-reduced, the grouped AUC's rows exchanged so that a group meets on the rank
`key % world` -- gives the single-process values: integers exactly, the grouped AUC at rtol 1e-12."""
import os
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def _worker(rank, world, init_file, emu_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    import metrics_ref as ref
    from test_sharded_gloo import _finish_worker
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.metrics import BinnedAUC, GroupedAUC, NormalizedEntropy

    _lib.use_library(emu_path)
    g = torch.Generator().manual_seed(21)
    n, steps = 301, 3  # (odd: the ranks' slices differ in length)
    p = torch.randint(0, 40, (steps, n), generator=g).to(torch.float32) / 39.0
    y = (torch.rand(steps, n, generator=g) < 0.35).to(torch.int64)
    k = torch.randint(-6, 7, (steps, n), generator=g) * ((1 << 33) + 1)  # 13 groups that span ranks and steps, negative keys too
    pg = dist.group.WORLD
    one = (BinnedAUC(200), NormalizedEntropy(), GroupedAUC(capacity=steps * n))
    mine = (BinnedAUC(200, process_group=pg), NormalizedEntropy(process_group=pg), GroupedAUC(capacity=steps * n, process_group=pg))
    cut = n // 3  # rank 0: the first third, rank 1: the rest
    sl = slice(0, cut) if rank == 0 else slice(cut, n)
    for s in range(steps):
        for m, rows in ((one, slice(0, n)), (mine, sl)):
            m[0].update(p[s, rows], y[s, rows])
            m[1].update(p[s, rows], y[s, rows])
            m[2].update(p[s, rows], y[s, rows], k[s, rows])
    assert torch.equal(mine[0].confmat(), one[0].confmat())
    assert torch.equal(mine[0].confmat(), ref.confmat(p.reshape(-1), y.reshape(-1), torch.linspace(0, 1, 200)))
    assert mine[0].compute().item() == one[0].compute().item()
    assert mine[1].state()[1:].tolist() == one[1].state()[1:].tolist() == [float(steps * n), float(y.sum())]
    torch.testing.assert_close(mine[1].compute(), one[1].compute(), rtol=1e-5, atol=0.0)
    want = ref.grouped_auc(p.reshape(-1), y.reshape(-1), k.reshape(-1))
    torch.testing.assert_close(one[2].compute(), torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(mine[2].compute(), torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0.0)
    dist.barrier()
    _finish_worker()


def test_metrics_over_two_ranks_equal_one_process(emu_path):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), emu_path), nprocs=2, join=True)
