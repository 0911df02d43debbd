"""tests/golden/mind_mini.config, variants of it by text replacement, and its synthetic batches, shared by the mind tests."""
import os

import numpy as np
import torch

from dssm_variants import with_line  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "mind_mini.config")).read()


def batches(spec, B, n, seed=0, fixed_total=False):
    """n host batches of B rows: user_id, age_level and the click history in the base data group, the item-side features in
    "__NEG__" with B + num_sample rows.  Histories of 0 .. sequence_length + 3 clicks (the capsule layer truncates), the first one
    empty, both sub-features of the block with the same lengths; fixed_total: every batch has the same multiset of lengths in
    another order, so its tensors have the same shapes (what a replayed graph needs)."""
    from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch
    from torcheasyrec_amd.match import NEG_DATA_GROUP
    from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor

    rng = np.random.default_rng(seed)
    by_name = {f.name: f for f in spec.features}
    item_names = list(spec.negative_sampler["attr_fields"])
    N = spec.negative_sampler["num_sample"]
    base = [f for f in spec.features if f.name not in item_names]
    assert all(f.is_sparse for f in base)
    smax = max(f.sequence_length for f in base if f.is_sequence) + 3
    multiset = rng.integers(0, smax + 1, size=B).astype(np.int32)
    out = []
    for _ in range(n):
        hist = rng.permutation(multiset) if fixed_total else rng.integers(0, smax + 1, size=B).astype(np.int32)
        if not fixed_total:
            hist[0] = 0
        lens = [hist if f.is_sequence else np.ones(B, np.int32) for f in base]
        ids = np.concatenate([rng.integers(0, f.num_embeddings, size=int(ln.sum())) for f, ln in zip(base, lens)]).astype(np.int64)
        all_lens = torch.from_numpy(np.concatenate(lens))
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), all_lens.to(torch.int64).cumsum(0)])  # (with the batch: a slot refreshes them in place)
        sparse = {BASE_DATA_GROUP: KeyedJaggedTensor([f.name for f in base], torch.from_numpy(ids), all_lens, None, offsets)}
        feats = [by_name[x] for x in item_names]
        sp, de = [f for f in feats if f.is_sparse], [f for f in feats if not f.is_sparse]
        nids = np.concatenate([rng.integers(0, f.num_embeddings, size=B + N) for f in sp]).astype(np.int64)
        sparse[NEG_DATA_GROUP] = KeyedJaggedTensor([f.name for f in sp], torch.from_numpy(nids), torch.ones(len(sp) * (B + N), dtype=torch.int32),
                                                   uniform_length=1)
        dense = {NEG_DATA_GROUP: KeyedTensor([f.name for f in de], [f.value_dim for f in de],
                                             torch.from_numpy(rng.random((B + N, sum(f.value_dim for f in de)), dtype=np.float32)))}
        out.append(Batch(dense, sparse, {name: torch.ones(B, dtype=torch.int64) for name in spec.label_fields}, {}))
    return out
