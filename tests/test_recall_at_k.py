"""metrics.RecallAtK (`recall_at_k { top_k }` of a match model) against the reference's rule restated here
(tzrec/metrics/recall_at_k.py:44-49: argsort the scores descending, keep the first k columns, gather the one-hot label, a hit
when any is set), on tie-free scores; accumulation over updates; the Evaluator's keys."""
import pytest
import torch

from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.match import IN_BATCH, SAMPLED, scores_loss_rank
from torcheasyrec_amd.metrics import Evaluator, RecallAtK


def reference_hits(sim, label, k):
    """recall_at_k.py:44-49"""
    onehot = torch.zeros_like(sim, dtype=torch.bool)
    onehot[torch.arange(sim.shape[0]), label] = True
    top = torch.argsort(sim, dim=1, descending=True)[:, :k]
    return torch.gather(onehot, 1, top).any(dim=1).sum().item()


def tie_free(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    sim = torch.randn(B, C, generator=g)
    assert all(len(set(row.tolist())) == C for row in sim)
    return sim


@pytest.mark.parametrize("mode,B,C", [(SAMPLED, 33, 13), (IN_BATCH, 17, 17), (SAMPLED, 5, 1)])
@pytest.mark.parametrize("k", [1, 5, 20])
def test_rank_rule_equals_the_references_argsort_gather(mode, B, C, k):
    sim = tie_free(B, C, seed=B + k)
    label = torch.arange(B) if mode == IN_BATCH else torch.zeros(B, dtype=torch.long)
    _, rank = scores_loss_rank(sim, mode)
    m = RecallAtK(k)
    m.update(rank)
    want = reference_hits(sim, label, k)
    assert m._state.dtype == torch.int64 and m._state.tolist() == [want, B]
    assert float(m.compute()) == pytest.approx(want / B)


def test_accumulates_over_three_updates_and_resets():
    m, hits, rows = RecallAtK(5), 0, 0
    for s, B in enumerate((9, 4, 16)):
        sim = tie_free(B, 13, seed=40 + s)
        m.update(scores_loss_rank(sim, SAMPLED)[1])
        hits += reference_hits(sim, torch.zeros(B, dtype=torch.long), 5)
        rows += B
    assert m._state.tolist() == [hits, rows] and float(m.compute()) == pytest.approx(hits / rows)
    m.reset()
    assert m._state.tolist() == [0, 0]
    with pytest.raises(ValueError, match="top_k"):
        RecallAtK(0)


def test_evaluator_builds_recall_at_k_under_the_references_keys():
    import dssm_variants as dv

    spec = load_pipeline_spec(dv.TEXT)

    class Stub:
        _pg = None

    ev = Evaluator(Stub(), spec, torch.device("cpu"))
    assert sorted(ev.metrics) == ["recall@1", "recall@5"] and [ev.metrics[n].top_k for n in sorted(ev.metrics)] == [1, 5]
    sim = tie_free(12, 13, seed=3)
    ev.update({"rank": scores_loss_rank(sim, SAMPLED)[1]}, None)
    out = ev.compute()
    assert 0.0 <= float(out["recall@1"]) <= float(out["recall@5"]) <= 1.0
    assert float(out["recall@5"]) == pytest.approx(reference_hits(sim, torch.zeros(12, dtype=torch.long), 5) / 12)
    twice = dv.with_line(dv.TEXT, "    metrics { recall_at_k { top_k: 5 } }\n", "    metrics { recall_at_k { top_k: 5 } }\n")
    with pytest.raises(ValueError, match="recall@5"):
        Evaluator(Stub(), load_pipeline_spec(twice), torch.device("cpu"))
