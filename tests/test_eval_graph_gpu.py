"""`evaluate(graph=True)`: forward and every metric update of tests/golden/deepfm_mini.config captured once and replayed per
batch, against the eager loop on the same batches -- integers and the grouped AUC exactly, NE within its tolerance (the
captured step runs the same kernels on the same values; only the double atomics' order is free)."""
import os

import pytest
import torch

from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import _lib
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.metrics import Evaluator, evaluate
from torcheasyrec_amd.rank_model import build_rank_model

pytestmark = pytest.mark.gpu
TEXT = open(os.path.join(os.path.dirname(__file__), "golden", "deepfm_mini.config")).read().replace(
    "metrics { auc {} }", 'metrics { auc {} } metrics { grouped_auc { grouping_key: "cat_1" } } metrics { normalized_entropy {} }')


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    _lib.use_native()
    dev = torch.device("cuda", 0)
    spec = load_pipeline_spec(TEXT)
    torch.manual_seed(7)
    model = build_rank_model(spec, device=dev)
    return dev, spec, model, list(synthetic_batches(spec, 3 * 256, 256, seed=8))


def test_graph_replay_equals_the_eager_loop(setup):
    dev, spec, model, batches = setup
    eager, graph = Evaluator(model, spec, dev), Evaluator(model, spec, dev)
    want = evaluate(model, batches, eager)
    got = evaluate(model, batches, graph, graph=True)
    assert int(eager.metrics["auc"].histogram().sum()) == 3 * 256
    assert torch.equal(graph.metrics["auc"].confmat(), eager.metrics["auc"].confmat())
    assert got["auc"].item() == want["auc"].item()
    for a, b in zip(graph.metrics["grouped_auc"].rows(), eager.metrics["grouped_auc"].rows()):
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    assert got["grouped_auc"].item() == want["grouped_auc"].item() and 0.0 <= got["grouped_auc"].item() <= 1.0
    assert graph.metrics["normalized_entropy"].state()[1:].tolist() == eager.metrics["normalized_entropy"].state()[1:].tolist()
    torch.testing.assert_close(got["normalized_entropy"], want["normalized_entropy"], rtol=1e-5, atol=0.0)


def test_graph_refuses_a_batch_whose_uniform_hints_differ(setup):
    dev, spec, model, batches = setup
    from torcheasyrec_amd.embedding_group import BASE_DATA_GROUP, Batch
    from torcheasyrec_amd.sparse import KeyedJaggedTensor

    k = batches[1].sparse_features[BASE_DATA_GROUP]
    lengths = k.lengths().clone()
    lengths[0], lengths[1] = 2, 0  # same sizes, no longer one id per bag
    odd = Batch(batches[1].dense_features, {BASE_DATA_GROUP: KeyedJaggedTensor(k.keys(), k.values(), lengths)}, batches[1].labels)
    with pytest.raises(ValueError, match="uniform-length hints"):
        evaluate(model, [batches[0], odd], Evaluator(model, spec, dev), graph=True)
    short = next(iter(synthetic_batches(spec, 100, 100, seed=9)))
    with pytest.raises(ValueError, match="fixed-shape"):
        evaluate(model, [batches[0], short], Evaluator(model, spec, dev), graph=True)
