#!/usr/bin/env python3
"""End to end on one MI355X from a tzrec text config: parse -> build the rank model (tables, groups,
fused sparse optimizer from the config) -> train on synthetic Criteo-shaped batches -> evaluate the config's `metrics` on
held-out batches (state on the device, torcheasyrec_amd/metrics.py).

    python examples/train_from_config.py tests/golden/deepfm_mini.config
    python examples/train_from_config.py tests/golden/mmoe_seq_mini.config     (a click history inside the DEEP group)
    python examples/train_from_config.py tests/golden/jrc_mini.config          (jrc_loss over sessions, a sample weight column)
    python examples/train_from_config.py tests/golden/dcn_mini.config          (dcn_v1: the cross network in one launch)
    python examples/train_from_config.py tests/golden/dcn_v2_mini.config       (dcn_v2: the low-rank cross network, one launch forward, two backward)
    python examples/train_from_config.py tests/golden/xdeepfm_mini.config      (xdeepfm: the CIN without its [B, H F, D] tensor)
    python examples/train_from_config.py tests/golden/masknet_mini.config      (mask_net: LayerNorm, masks and concat in two row launches)
    python examples/train_from_config.py tests/golden/wukong_mini.config       (wukong: each layer's FM front and mix in one launch each)
    python examples/train_from_config.py tests/golden/ple_mini.config          (ple: every gate of a CGC level mixed in one launch; per-tower metrics)
    python examples/train_from_config.py tests/golden/pepnet_mini.config       (pepnet: EPNet / PPNet gates in one launch per level; a tower per task and domain)
    python examples/train_from_config.py tests/golden/dbmtl_mini.config        (dbmtl: every Bayesian relation tower in one launch, no concat tensor)
    python examples/train_from_config.py tests/golden/dssm_mini.config         (dssm: a match model; sampled softmax without its score matrix, recall@k)
    python examples/train_from_config.py tests/golden/mind_mini.config         (mind: a click history routed into interests in one launch, label-aware attention)
    python examples/train_from_config.py tests/golden/dat_mini.config          (dat: augment groups beside the towers' own, the Adaptive-Mimic loss of both sides in one launch)
    python examples/train_from_config.py tests/golden/rocket_mini.config       (rocket_launching: a booster and a light net, every distillation term of a step in one launch; auc_light)

What a tzrec user keeps: the pipeline config, feature / group / model semantics, `pipeline.progress`.
What changes underneath: the embedding path runs on libtzrec_hip.so."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.config import load_pipeline_spec  # noqa: E402
from torcheasyrec_amd.dense_optim import build_dense_optimizer, create_dense_schedulers, named_dense_parameters  # noqa: E402
from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch, TrainPipeline  # noqa: E402
from torcheasyrec_amd.lr_scheduler import create_scheduler  # noqa: E402
from torcheasyrec_amd.rank_model import build_rank_model  # noqa: E402
from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor  # noqa: E402


NEG_DATA_GROUP = "__NEG__"  # tzrec/datasets/utils.py:29


def synthetic_batches(spec, n_rows, batch_size, seed=0):
    rng = np.random.default_rng(seed)
    # data_config.negative_sampler (a match model): the item-side features it names in `attr_fields` travel in a data group of
    # their own, "__NEG__", with batch + num_sample rows -- row i the positive of sample i, the rest negatives for the whole
    # batch -- all drawn uniformly here.  This stands in for the reference's graph sampler (tzrec/datasets/sampler.py), which
    # draws the negatives by item weight from its `input_path` table.
    sampler = getattr(spec, "negative_sampler", None)
    item_side = set(sampler["attr_fields"]) if sampler else set()
    neg = [f for f in spec.features if f.name in item_side]
    sparse = [f for f in spec.features if f.is_sparse and f.name not in item_side]
    dense = [f for f in spec.features if not f.is_sparse and f.name not in item_side]
    for s in range(0, n_rows, batch_size):
        b = min(batch_size, n_rows - s)
        # one id per sample, except the sub-features of a `sequence_feature` block: a history of 0 .. sequence_length ids, the
        # same lengths for every sub-feature of one block
        seq_lens = {}
        lens = [seq_lens.setdefault(f.name.split("__")[0], rng.integers(0, (f.sequence_length or 8) + 1, size=b).astype(np.int32))
                if f.is_sequence else np.ones(b, np.int32) for f in sparse]
        ids = np.concatenate([rng.integers(0, f.num_embeddings, size=int(ln.sum())) for f, ln in zip(sparse, lens)]).astype(np.int64)
        kjt = KeyedJaggedTensor([f.name for f in sparse], torch.from_numpy(ids), torch.from_numpy(np.concatenate(lens)),
                                uniform_length=None if seq_lens else 1)
        kt = KeyedTensor([f.name for f in dense], [f.value_dim for f in dense],
                         torch.from_numpy(rng.random((b, sum(f.value_dim for f in dense)), dtype=np.float32)))
        labels = {name: torch.from_numpy((rng.random(b) < 0.25).astype(np.int64)) for name in spec.label_fields}
        # data_config.sample_weight_fields: one float column each (the losses read them, torcheasyrec_amd/losses.py)
        weights = {name: torch.from_numpy((0.5 + rng.random(b)).astype(np.float32)) for name in spec.sample_weight_fields}
        dense_groups, sparse_groups = {BASE_DATA_GROUP: kt}, {BASE_DATA_GROUP: kjt}
        if sampler:
            rows = b + int(sampler["num_sample"])
            nsp, nde = [f for f in neg if f.is_sparse], [f for f in neg if not f.is_sparse]
            if nsp:
                nids = np.concatenate([rng.integers(0, f.num_embeddings, size=rows) for f in nsp]).astype(np.int64)
                sparse_groups[NEG_DATA_GROUP] = KeyedJaggedTensor([f.name for f in nsp], torch.from_numpy(nids),
                                                                  torch.ones(len(nsp) * rows, dtype=torch.int32), uniform_length=1)
            if nde:
                dense_groups[NEG_DATA_GROUP] = KeyedTensor([f.name for f in nde], [f.value_dim for f in nde],
                                                           torch.from_numpy(rng.random((rows, sum(f.value_dim for f in nde)), dtype=np.float32)))
        yield Batch(dense_groups, sparse_groups, labels, weights)


def main(path):
    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(open(path).read())
    model = build_rank_model(spec, device=dev)
    # train_config.dense_optimizer: its kind with every field, its part_optimizers as groups of the same one-launch step
    # (tzrec/optim/optimizer_builder.py:100-260)
    opt = build_dense_optimizer(named_dense_parameters(model), spec.dense_optimizer)
    # the `learning_rate` oneof of the two optimizer blocks and of every part (tzrec/main.py:877-882); stepped per step
    # unless by_epoch (main.py:542-544)
    # (a match model has an embedding group, and so a fused sparse optimizer, per tower: `fused_optimizers`)
    fused = model.fused_optimizers if hasattr(model, "fused_optimizers") else [model.fused_optimizer]
    schedulers = [create_scheduler(fo, spec.sparse_optimizer_block) for fo in fused] + create_dense_schedulers(opt, spec.dense_optimizer)
    # train_config.grad_clipping / gradient_accumulation_steps around the dense optimizer (tzrec/main.py:848-876)
    from torcheasyrec_amd.optimizer import build_train_optimizer

    pipe = TrainPipeline(model, build_train_optimizer(opt, spec.grad_clipping, spec.gradient_accumulation_steps), dev, model.loss)
    # train_config.delta_embedding_dump_config: the call sites of tzrec/main.py:805-811,900,547,611,928
    dumper = None
    if spec.delta_embedding_dump_config is not None:
        from torcheasyrec_amd.delta_embedding_dump import DeltaEmbeddingDumper

        dumper = DeltaEmbeddingDumper(model, spec.delta_embedding_dump_config, os.environ.get("MODEL_DIR", "experiments/model"), dev)
        dumper.start()
    it = iter(synthetic_batches(spec, 20 * (spec.batch_size or 1024), spec.batch_size or 1024))
    step = 0
    while True:
        try:
            losses, preds, _ = pipe.progress(it)
        except StopIteration:
            break
        step += 1
        for sch in schedulers:
            if not sch.by_epoch:
                sch.step()
        if dumper is not None:
            dumper.maybe_dump(step)
        if step % 5 == 0:
            print(f"step {step}: " + ", ".join(f"{k}={float(v.detach()):.4f}" for k, v in losses.items()))
    if dumper is not None:
        print("delta embedding dump:", dumper.final_dump(step))
        dumper.close()
    if hasattr(model, "embedding_group"):
        print("tables:", {n: tuple(w.shape) for n, w in model.embedding_group.ebc.table_weights().items()})
    else:  # a match model: each tower's own
        print("tables:", {f"{t}.{n}": tuple(w.shape) for t in ("user_tower", "item_tower")
                          for n, w in getattr(model, t).embedding_group.ebc.table_weights().items()})
    # model_config.metrics (and every task tower's) on a held-out run of batches: the evaluate half of the reference's
    # train_and_evaluate (tzrec/main.py).  EVAL_GRAPH=1: forward and metric updates replayed from one hipGraph
    if spec.metrics:
        from torcheasyrec_amd.metrics import Evaluator, evaluate

        bs = spec.batch_size or 1024
        held_out = synthetic_batches(spec, int(os.environ.get("EVAL_BATCHES", "8")) * bs, bs, seed=1)
        result = evaluate(model, held_out, Evaluator(model, spec, dev), graph=os.environ.get("EVAL_GRAPH", "0") == "1")
        print("eval:", {k: round(float(v), 6) for k, v in result.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "deepfm_mini.config"))
