"""A few train steps of the mini config scaled to mmoe_has_sequence's shapes: B = 8192, histories of up to 50 clicks, three
16-wide sequence features (D = 48).  Run under rocprofv3 --kernel-trace --stats."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from torcheasyrec_amd import _lib  # noqa: E402
from torcheasyrec_amd.config import load_pipeline_spec  # noqa: E402
from torcheasyrec_amd.dense import FusedDenseAdam  # noqa: E402
from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch, _backward_of_losses, _losses_and_predictions  # noqa: E402
from torcheasyrec_amd.rank_model import build_rank_model  # noqa: E402
from torcheasyrec_amd.sparse import KeyedJaggedTensor, KeyedTensor  # noqa: E402

text = open(os.path.join(ROOT, "tests", "golden", "mmoe_seq_mini.config")).read()
text = text.replace("sequence_length: 8", "sequence_length: 50")
text = text.replace('feature_configs { id_feature { feature_name: "cate_id" num_buckets: 40 embedding_dim: 16 } }',
                    'feature_configs { id_feature { feature_name: "cate_id" num_buckets: 12961 embedding_dim: 16 } }\n'
                    'feature_configs { id_feature { feature_name: "brand" num_buckets: 461498 embedding_dim: 16 } }')
text = text.replace('        features { id_feature { feature_name: "cate_id" num_buckets: 40 embedding_dim: 16 } }',
                    '        features { id_feature { feature_name: "cate_id" num_buckets: 12961 embedding_dim: 16 } }\n'
                    '        features { id_feature { feature_name: "brand" num_buckets: 461498 embedding_dim: 16 } }')
text = text.replace("num_buckets: 300", "num_buckets: 846812").replace("num_buckets: 500", "num_buckets: 1141730")
text = text.replace('        feature_names: "cate_id"\n        feature_names: "price"', '        feature_names: "cate_id"\n        feature_names: "brand"\n        feature_names: "price"')
text = text.replace('            feature_names: "cate_id"\n            feature_names: "click_seq__adgroup_id"\n            feature_names: "click_seq__cate_id"',
                    '            feature_names: "cate_id"\n            feature_names: "brand"\n            feature_names: "click_seq__adgroup_id"\n'
                    '            feature_names: "click_seq__cate_id"\n            feature_names: "click_seq__brand"')
text = text.replace("hidden_units: [8, 4]", "hidden_units: [32, 8]")
spec = load_pipeline_spec(text)
_lib.use_native()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = build_rank_model(spec, device=dev)
eg = model.embedding_group
assert eg.jagged_sequence_groups == {"click_seq"} and eg.group_total_dim("click_seq.sequence") == 48, (eg.jagged_sequence_groups,)
opt = FusedDenseAdam(list(model.dense_parameters()), lr=1e-3)
B = 8192
rng = np.random.default_rng(0)
sparse = [f for f in spec.features if f.is_sparse]
dense = [f for f in spec.features if not f.is_sparse]


def batch():
    seq = rng.integers(0, 51, size=B).astype(np.int32)
    lens = [seq if f.is_sequence else np.ones(B, np.int32) for f in sparse]
    vals = np.concatenate([rng.integers(0, f.num_embeddings, size=int(ln.sum())) for f, ln in zip(sparse, lens)]).astype(np.int64)
    kjt = KeyedJaggedTensor([f.name for f in sparse], torch.from_numpy(vals), torch.from_numpy(np.concatenate(lens)))
    kt = KeyedTensor([f.name for f in dense], [f.value_dim for f in dense], torch.from_numpy(rng.random((B, len(dense)), dtype=np.float32)))
    return Batch({BASE_DATA_GROUP: kt}, {BASE_DATA_GROUP: kjt}, {n: torch.from_numpy((rng.random(B) < 0.3).astype(np.int64)) for n in spec.label_fields}).to(dev), int(seq.sum())


for i in range(8):
    b, n = batch()
    opt.zero_grad(set_to_none=True)
    losses, _ = _losses_and_predictions(model, model.loss, b)
    _backward_of_losses(losses)
    opt.step()
torch.cuda.synchronize()
print("positions in the last batch:", n, "losses", {k: float(v) for k, v in losses.items()})
