"""The sharded collections on ONE rank with mean-pooled tables, per-id weights and lookups that feed two and three feature groups:
every kernel and every collective call of the exchange executes (the all-to-alls are self copies), so each step must equal the
oracle's pooled_lookup / lookup_grads / sparse_update with each table's own pooling.  The `hip` variant runs through a
world-size-1 RCCL group on the GPU; the `emu` variant is the same body over gloo + the lane emulator
(tests/test_zz_mixed_sharded_world1.py).

(Named test_zz_* like that file, so that it sorts last: the `hip` variant creates and destroys its RCCL group inside the pytest
process, and an abort on that group's watchdog thread takes the whole session with it wherever the main thread happens to be
-- tests/test_sharded_gpu.py::_isolated.  Behind it nothing is left to take down.)

Upstream gradients are standard normal over B, the scale of a mean-reduced loss, at which the weight tolerance (rtol 1e-5, atol
1e-7: tests/test_sharded_gloo.py, tests/test_zz_mixed_sharded_world1.py) was set in this project: the accumulator's 0.1 then
dominates g^2, the Adagrad step is lr g / sqrt(0.1) to first order, and the order in which a row's n duplicate ids are added
(the oracle: lookup order; the kernels: sorted) moves a weight by at most 0.32 n 2^-24 sum |g_i| -- 2e-8 at B = 256 on the 50-row
table (n about 12, |g_i| about 7e-3).  With gradients of unit scale the same order of addition alone moves near-cancelling sums
by 1.4e-7 on an MI355X (measured: one element of 800 of the 50-row table after the first step), which says nothing about the
kernels.  Largest weight difference over the eight steps (printed per step and table): 1.1e-8 on the lane emulator at B = 24,
1.5e-8 on an MI355X at B = 256.

The requester-side backward kernel, tzr_lookup_grads, is reached here with its mean-pooling divide, its per-id weights and its
sum over two and three groups; tests/test_lookup_grads.py calls it directly."""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle import tzrec_oracle as orc  # noqa: E402

D = 16
KEYS = ["a", "b", "c", "d"]
ROWS = {"a": 50, "b": 301, "c": 120, "d": 7}
POOL = {"a": "mean", "b": "mean", "c": "sum", "d": "mean"}
GROUPS = {"fm": ["a", "b"], "deep": ["a", "b", "c", "d"], "third": ["c", "a"]}
LR, ACC0 = 0.1, 0.1
# (ragged bags of 0..4 ids, per-id weights)
STEPS = [(False, False), (True, False), (True, True), (False, True)]


def _seeded(t):
    def f(w):
        g = torch.Generator().manual_seed(100 + t)
        w.copy_((torch.rand(w.shape, generator=g) - 0.5) * 0.2)
    return f


def _count_lookup_grads():
    """calls of tzr_lookup_grads since this call (tests/test_cin.py::_count_calls)"""
    from torcheasyrec_amd import _lib

    lib, n = _lib.lib(), [0]
    orig = lib.tzr_lookup_grads

    def f(*a):
        n[0] += 1
        return orig(*a)

    lib.tzr_lookup_grads = f

    def done():
        lib.tzr_lookup_grads = orig
        return n[0]

    return done


def _batch(rng, B, ragged, weighted, dev):
    from torcheasyrec_amd.sparse import KeyedJaggedTensor

    F = len(KEYS)
    lens = rng.integers(0, 5, size=(F, B)).astype(np.int32) if ragged else np.ones((F, B), dtype=np.int32)
    if ragged:
        lens[:, 0], lens[:, 1] = 0, 1  # an empty bag and a mean bag of one id in every table
    vals = np.concatenate([rng.integers(0, ROWS[k], size=int(lens[f].sum())) for f, k in enumerate(KEYS)]).astype(np.int64)
    wts = rng.uniform(0.5, 1.5, size=len(vals)).astype(np.float32) if weighted else None
    kjt = KeyedJaggedTensor(KEYS, torch.from_numpy(vals), torch.from_numpy(lens.reshape(-1)), None if wts is None else torch.from_numpy(wts),
                            uniform_length=None if ragged else 1)
    return kjt.to(dev), vals, lens.reshape(-1), wts


def _train(sh, ref, dev, B, seed):
    """four steps of `sh` next to the oracle; `ref`: the unsharded collection, for the first step's bit-equal forward"""
    cfg = orc.SparseOptim(kind="adagrad", lr=LR)
    w = {k: sh.table_weights()[f"t_{k}"].detach()[:ROWS[k]].cpu().numpy().copy() for k in KEYS}
    m = {k: np.full_like(w[k], ACC0) for k in KEYS}
    rng = np.random.default_rng(seed)
    calls = _count_lookup_grads()
    try:
        for step, (ragged, weighted) in enumerate(STEPS):
            kjt, vals, lens, wts = _batch(rng, B, ragged, weighted, dev)
            off = orc.lengths_to_offsets(lens)
            out = sh.forward_grouped(kjt)
            # forward: the oracle on the rows the collection holds now
            held = [sh.table_weights()[f"t_{k}"].detach()[:ROWS[k]].cpu().clone() for k in KEYS]
            blocks = dict(zip(KEYS, orc.pooled_lookup(held, [POOL[k] for k in KEYS], torch.from_numpy(vals), torch.from_numpy(lens), B,
                                                      None if wts is None else torch.from_numpy(wts))))
            for g, want in orc.regroup(blocks, GROUPS).items():
                assert out[g].shape == (B, D * len(GROUPS[g]))
                torch.testing.assert_close(out[g].detach().cpu(), want, rtol=1e-6, atol=1e-7, msg=lambda s, g=g: f"step {step} {g}: {s}")
            if step == 0:  # one unweighted id per bag: a copy on both paths, whatever the pooling
                out_ref = ref.forward_grouped(kjt)
                for g in GROUPS:
                    assert torch.equal(out[g].detach(), out_ref[g].detach()), g
            up = {g: torch.randn(B, D * len(ks), generator=torch.Generator().manual_seed(seed + 10 * step + i)) / B
                  for i, (g, ks) in enumerate(GROUPS.items())}
            sum((out[g] * up[g].to(dev)).sum() for g in GROUPS).backward()
            # backward: the groups' gradient slices of a lookup summed, then one row per id, then the fused Adagrad
            for f, k in enumerate(KEYS):
                gb = sum(up[g][:, D * ks.index(k):D * (ks.index(k) + 1)].numpy() for g, ks in GROUPS.items() if k in ks)
                lo, hi = int(off[f * B]), int(off[(f + 1) * B])
                lg = orc.lookup_grads([gb], lens[f * B:(f + 1) * B], B, [POOL[k]], None if wts is None else wts[lo:hi])
                orc.sparse_update(w[k], m[k], vals[lo:hi], lg, cfg)
                got = sh.table_weights()[f"t_{k}"].detach()[:ROWS[k]].cpu().numpy()
                diff = float(np.abs(got - w[k]).max())
                print(f"sharded pooling on {dev.type}: step {step} table {k} ({POOL[k]}): largest weight difference {diff:.3g}")
                np.testing.assert_allclose(got, w[k], rtol=1e-5, atol=1e-7, err_msg=f"step {step} table {k}")
    finally:
        n = calls()
    assert n == len(STEPS)  # the requester-side backward ran, once per step


def test_mean_pooling_weights_and_shared_lookups_on_one_rank(dev):
    from torcheasyrec_amd.embedding import EmbeddingBagCollection, EmbeddingBagConfig, SparseOptimizerConfig
    from torcheasyrec_amd.sharding import MixedShardedEmbeddingBagCollection, ShardedEmbeddingBagCollection

    cfgs = lambda: [EmbeddingBagConfig(f"t_{k}", D, ROWS[k], [k], POOL[k], init_fn=_seeded(t)) for t, k in enumerate(KEYS)]  # noqa: E731
    assert sorted(POOL.values()) == ["mean", "mean", "mean", "sum"]
    assert sorted(sum(k in ks for ks in GROUPS.values()) for k in KEYS) == [1, 2, 2, 3]  # lookups feed up to three groups
    opt = SparseOptimizerConfig(kind="adagrad", lr=LR, initial_accumulator_value=ACC0)
    B = 256 if dev.type == "cuda" else 24
    with tempfile.TemporaryDirectory() as d:
        if dev.type == "cuda":
            dist.init_process_group("nccl", init_method=f"file://{d}/init", rank=0, world_size=1, device_id=dev)
        else:
            dist.init_process_group("gloo", init_method=f"file://{d}/init", rank=0, world_size=1)
        try:
            ref = EmbeddingBagCollection(cfgs(), device=dev, optimizer=opt, groups=GROUPS)
            # every table row-wise (one lane: one dim, no feature twice)
            sh = MixedShardedEmbeddingBagCollection(cfgs(), device=dev, optimizer=opt, groups=GROUPS)
            assert len(sh.lanes) == 1 and {p["sharding_type"] for p in sh.plan().values()} == {"row_wise"}
            _train(sh, ref, dev, B, seed=1)
            # the 7-row table replicated: its backward (row sums, all-reduce, dense update) next to the row-wise one, under mean pooling
            sh2 = ShardedEmbeddingBagCollection(cfgs(), device=dev, optimizer=opt, groups=GROUPS, dp_max_rows=10, replicate_at_world1=True)
            kinds = {n: p["sharding_type"] for n, p in sh2.plan().items()}
            assert kinds == {"t_a": "row_wise", "t_b": "row_wise", "t_c": "row_wise", "t_d": "data_parallel"} and POOL["d"] == "mean"
            _train(sh2, ref, dev, B, seed=2)
        finally:
            dist.destroy_process_group()
