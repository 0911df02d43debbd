"""tests/golden/mmoe_seq_mini.config over two gloo ranks (CPU, the lane emulator): the DEEP group's tensor -- own features plus
the three sequence encoders over the nested group's sharded unpooled tables -- on my slice equals the unsharded model's on the
same samples, and after one step the sequence tables' rows end where the unsharded model's end on the global batch (the
comparison tests/test_sharded_gloo.py::_config_worker makes for sequence collections, same tolerances)."""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def _worker(rank, world, init_file, emu_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    from test_sharded_gloo import _finish_worker
    from torcheasyrec_amd import _lib
    from torcheasyrec_amd.config import load_pipeline_spec
    from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch
    from torcheasyrec_amd.rank_model import build_rank_model
    from torcheasyrec_amd.sharding import make_plan
    from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor

    _lib.use_library(emu_path)
    dev = torch.device("cpu")
    spec = load_pipeline_spec(open(os.path.join(os.path.dirname(__file__), "golden", "mmoe_seq_mini.config")).read())
    torch.manual_seed(11)
    ref = build_rank_model(spec, device=dev)
    torch.manual_seed(11)
    plan = make_plan(ref.embedding_group.ebc.embedding_bag_configs(), world, dp_max_rows=50)
    shd = build_rank_model(spec, device=dev, process_group=dist.group.WORLD, plan=plan)
    assert shd.embedding_group.jagged_sequence_groups == {"click_seq"}
    for name, w in ref.embedding_group.ebc.table_weights().items():  # same starting tables: the reference's rows into my shards
        lo, n = shd.embedding_group.ebc.shard_of(name)
        shd.embedding_group.ebc.table_weights()[name].data[:n].copy_(w.data[lo:lo + n])
    for d, ec in ref.embedding_group.ecs.items():
        sec = shd.embedding_group.ecs[d]
        for name, w in ec.table_weights().items():
            lo, n = sec.sharded.shard_of(name)
            sec.table_weights()[name].data[:n].copy_(w.data[lo:lo + n])
    dense_ref, dense_shd = list(ref.dense_parameters()), list(shd.dense_parameters())
    assert len(dense_ref) == len(dense_shd) and any(p is ref.embedding_group._group_name_to_seq_encoders["all"][0].linear.weight for p in dense_ref)
    for pr, ps in zip(dense_ref, dense_shd):
        ps.data.copy_(pr.data)
    sparse = [f for f in spec.features if f.is_sparse]
    dense = [f for f in spec.features if not f.is_sparse]
    Bl = 10
    parts = []
    for r in range(world):
        rng = np.random.default_rng(40 + r)
        seq = rng.integers(0, 10, size=Bl).astype(np.int32)  # up to 9 clicks: one more than sequence_length
        seq[:2] = [0, 8]
        lens = [seq if f.is_sequence else np.ones(Bl, np.int32) for f in sparse]
        parts.append(([rng.integers(0, f.num_embeddings, size=int(ln.sum())) for f, ln in zip(sparse, lens)], lens,
                      rng.random((Bl, len(dense)), dtype=np.float32), {l: (rng.random(Bl) < 0.4).astype(np.int64) for l in spec.label_fields}))

    def batch_of(rs):
        vals = [np.concatenate([parts[r][0][i] for r in rs]) for i in range(len(sparse))]
        lens = [np.concatenate([parts[r][1][i] for r in rs]) for i in range(len(sparse))]
        kjt = KeyedJaggedTensor([f.name for f in sparse], torch.from_numpy(np.concatenate(vals).astype(np.int64)), torch.from_numpy(np.concatenate(lens)))
        kt = KeyedTensor([f.name for f in dense], [f.value_dim for f in dense], torch.from_numpy(np.concatenate([parts[r][2] for r in rs])))
        return Batch({BASE_DATA_GROUP: kt}, {BASE_DATA_GROUP: kjt}, {l: torch.from_numpy(np.concatenate([parts[r][3][l] for r in rs])) for l in spec.label_fields})

    mine, full = batch_of([rank]), batch_of(list(range(world)))
    with torch.no_grad():
        got, want = shd.embedding_group(mine)["all"], ref.embedding_group(full)["all"][rank * Bl:(rank + 1) * Bl]
    assert got.shape[1] == 49 + 3 * 32
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
    ps, pr = shd(mine), ref(full)
    sum(shd.loss(ps, mine).values()).backward()
    shd.allreduce_dense_grads()
    ref_loss = 0
    for r in range(world):  # (the reference applies the SUM of the per-rank mean losses: tests/test_sharded_gloo.py)
        sub = {k: v[r * Bl:(r + 1) * Bl] for k, v in pr.items()}
        ref_loss = ref_loss + sum(ref.loss(sub, Batch({}, {}, {l: full.labels[l][r * Bl:(r + 1) * Bl] for l in spec.label_fields})).values())
    ref_loss.backward()
    for qs, qr in zip(dense_shd, dense_ref):
        torch.testing.assert_close(qs.grad, qr.grad / world, rtol=1e-4, atol=1e-6)
    compared = 0
    for d, ec in ref.embedding_group.ecs.items():
        sec = shd.embedding_group.ecs[d]
        for name, w in ec.table_weights().items():
            lo, n = sec.sharded.shard_of(name)
            if n:
                torch.testing.assert_close(sec.table_weights()[name].detach()[:n], w.detach()[lo:lo + n], rtol=2e-4, atol=1e-4, msg=name)
                compared += 1
    assert compared > 0
    dist.barrier()
    _finish_worker()


def test_sequence_encoders_in_a_deep_group_world2(emu_path):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), emu_path), nprocs=2, join=True)
