"""Variants of tests/golden/dssm_mini.config by text replacement, and its synthetic batches, shared by the dssm tests."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "dssm_mini.config")).read()

SAMPLER = TEXT[TEXT.index("    negative_sampler {"):TEXT.index("        item_id_field: \"adgroup_id\"\n    }\n") + len("        item_id_field: \"adgroup_id\"\n    }\n")]


def in_batch(text=TEXT):
    """no sampler, `in_batch_negative: true`: the other rows of the batch are the negatives"""
    assert text.count(SAMPLER) == 1 and text.count("        temperature: 0.05\n") == 1
    return text.replace(SAMPLER, "").replace("        temperature: 0.05\n", "        temperature: 0.05\n        in_batch_negative: true\n")


def with_line(text, anchor, line):
    """`line` put behind the one occurrence of `anchor`"""
    assert text.count(anchor) == 1, anchor
    return text.replace(anchor, anchor + line)


def batches(spec, B, n, seed=0, weights=False):
    """n host batches of B rows: the user-side features in the base data group; the item-side ones in "__NEG__" with B +
    num_sample rows under a negative sampler, else in the base group with B rows.  One id per bag."""
    from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch
    from torcheasyrec_amd.match import NEG_DATA_GROUP
    from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor

    rng = np.random.default_rng(seed)
    by_name = {f.name: f for f in spec.features}
    item_names = set(spec.negative_sampler["attr_fields"]) if spec.negative_sampler else set()
    N = spec.negative_sampler["num_sample"] if spec.negative_sampler else 0
    out = []
    for _ in range(n):
        dense, sparse = {}, {}
        for group, rows, feats in ((BASE_DATA_GROUP, B, [f for f in spec.features if f.name not in item_names]),
                                   (NEG_DATA_GROUP, B + N, [by_name[x] for x in spec.negative_sampler["attr_fields"]] if item_names else [])):
            sp, de = [f for f in feats if f.is_sparse], [f for f in feats if not f.is_sparse]
            if sp:
                ids = np.concatenate([rng.integers(0, f.num_embeddings, size=rows) for f in sp]).astype(np.int64)
                sparse[group] = KeyedJaggedTensor([f.name for f in sp], torch.from_numpy(ids), torch.ones(len(sp) * rows, dtype=torch.int32),
                                                  uniform_length=1)
            if de:
                dense[group] = KeyedTensor([f.name for f in de], [f.value_dim for f in de],
                                           torch.from_numpy(rng.random((rows, sum(f.value_dim for f in de)), dtype=np.float32)))
        labels = {name: torch.ones(B, dtype=torch.int64) for name in spec.label_fields}
        sw = {name: torch.from_numpy((0.5 + rng.random(B)).astype(np.float32)) for name in spec.sample_weight_fields} if weights else {}
        out.append(Batch(dense, sparse, labels, sw))
    return out
