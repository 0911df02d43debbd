"""`pepnet {...}` from its config (tests/golden/pepnet_mini.config): the model the reference builds from the same file
(tzrec/models/pepnet.py:27-245), the gate-and-scale step of EPNet and of each PPNet level on csrc/gate_scale.hip, the
per-sample choice among a task's domain towers as a mask-and-sum."""
import os
import types

import numpy as np
import pytest
import torch

from cross_v2_ref import FLOOR, rel_err
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import _lib, personalized_net
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.dense import FusedDenseAdam
from torcheasyrec_amd.metrics import BinnedAUC, Evaluator, evaluate, metric_update
from torcheasyrec_amd.personalized_net import EPNet, PPNet
from torcheasyrec_amd.rank_model import ConfigPEPNet, MultiTaskRankModel, build_rank_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "pepnet_mini.config")).read()
DOMAINS = '        domain_input_name: "dom"\n        task_domain_num: 2\n'
HIDDEN = "        ppnet_hidden_units: [32, 24]\n"


def _group(name):
    head = f'    feature_groups {{\n        group_name: "{name}"\n'
    start = TEXT.index(head)
    return TEXT[start:TEXT.index("    }\n", start) + len("    }\n")]


def _variant(epnet=True, ppnet=True, domains=True, text=TEXT):
    assert text.count(DOMAINS) == 1 and text.count(HIDDEN) == 1
    if not epnet:
        text = text.replace(_group("domain"), "")
    if not ppnet:
        text = text.replace(_group("uia"), "").replace(HIDDEN, "")
    if not domains:
        text = text.replace(DOMAINS, "")
    return text


def _model(dev, seed=0, text=TEXT):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=dev)


@pytest.fixture
def fwd_calls():
    calls = {"n": 0, "lib": None, "orig": None}

    def arm():
        L = _lib.lib()
        calls["lib"], calls["orig"] = L, L.tzr_gate_scale_fwd

        def counted(*a):
            calls["n"] += 1
            return calls["orig"](*a)

        L.tzr_gate_scale_fwd = counted
        return calls

    yield arm
    if calls["lib"] is not None:
        calls["lib"].tzr_gate_scale_fwd = calls["orig"]


def test_config_builds_the_references_model(dev):
    spec, model = _model(dev)
    assert spec.model_name == "pepnet" and type(model) is ConfigPEPNet and isinstance(model, MultiTaskRankModel)
    eg = model.embedding_group
    assert (eg.group_total_dim("all"), eg.group_total_dim("domain"), eg.group_total_dim("uia")) == (48, 17, 33)
    assert isinstance(model.epnet, EPNet) and isinstance(model.ppnet, PPNet)
    assert model.epnet.gate_nu.dense_layers[0].weight.shape == (20, 65) and model.epnet.gate_nu.dense_layers[2].weight.shape == (48, 20)
    assert model.epnet.gate_nu._gamma == 2.0 and model.ppnet._gamma == 2.0
    assert [tuple(l.weight.shape) for l in model.ppnet.linears] == [(32, 48), (24, 32)] * 2
    assert [tuple(g.dense_layers[0].weight.shape) for g in model.ppnet.gate_nus] == [(32, 81), (24, 81)] * 2
    # two towers per task, task * D + domain
    assert len(model.task_mlps) == len(model.task_outputs) == 4 and model.task_mlps[3].mlp[0].in_features == 24
    keys = {k for k in model.state_dict() if not k.startswith("embedding_group.")}
    assert {k.split(".")[0] for k in keys} == {"epnet", "ppnet", "task_mlps", "task_outputs"}
    assert "epnet.gate_nu.dense_layers.2.bias" in keys and "ppnet.gate_nus.3.dense_layers.0.weight" in keys and "ppnet.linears.3.bias" in keys
    assert len(list(model.dense_parameters())) == len(keys) == 4 + 4 * 6 + 4 * 6


def test_prediction_keys_are_the_references(dev):
    spec, model = _model(dev, seed=1)
    batch = next(synthetic_batches(spec, 20, 20, seed=2)).to(dev)
    with torch.no_grad():
        out = model(batch)
    assert sorted(out) == sorted(f"{kind}_{tower}_{d}" for kind in ("logits", "probs") for tower in ("ctr", "cvr") for d in (0, 1))
    assert all(v.shape == (20,) for v in out.values())
    assert sorted(model.select_domain_predictions(out, batch)) == ["logits_ctr", "logits_cvr", "probs_ctr", "probs_cvr"]
    spec, model = _model(dev, seed=1, text=_variant(domains=False))
    with torch.no_grad():
        out = model(batch)
    assert sorted(out) == ["logits_ctr", "logits_cvr", "probs_ctr", "probs_cvr"] and len(model.task_outputs) == 2
    assert model.select_domain_predictions(out, batch) is out


@pytest.mark.parametrize("epnet,ppnet", [(True, False), (False, True), (False, False), (True, True)])
def test_the_four_variants_build_and_run_a_step(dev, fwd_calls, epnet, ppnet):
    calls = fwd_calls()
    spec, model = _model(dev, seed=2, text=_variant(epnet=epnet, ppnet=ppnet))
    assert (model.epnet is not None) == epnet and (model.ppnet is not None) == ppnet
    assert model.task_mlps[0].mlp[0].in_features == (24 if ppnet else 48)  # without PPNet every tower reads the EPNet output / the main tensor
    opt = FusedDenseAdam(list(model.dense_parameters()), lr=0.01)
    batch = next(synthetic_batches(spec, 40, 40, seed=3)).to(dev)
    loss = model.loss(model(batch), batch)
    assert sorted(loss) == ["binary_cross_entropy_ctr", "binary_cross_entropy_cvr"]
    opt.zero_grad()
    (loss["binary_cross_entropy_ctr"] + loss["binary_cross_entropy_cvr"]).backward()
    assert calls["n"] == (1 if epnet else 0) + (2 if ppnet else 0)  # one launch per EPNet, one per PPNet level
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.dense_parameters())
    opt.step()
    assert all(bool(torch.isfinite(v).all()) for v in model(batch).values())


def test_configs_the_reference_cannot_run_are_refused(dev):
    with pytest.raises(ValueError, match="'all'"):
        _model(dev, text=TEXT.replace('group_name: "all"', 'group_name: "main"'))
    with pytest.raises(ValueError, match="ppnet_hidden_units"):
        _model(dev, text=TEXT.replace(HIDDEN, ""))
    with pytest.raises(ValueError, match="ppnet_dropout_ratio"):
        _model(dev, text=TEXT.replace(HIDDEN, HIDDEN + "        ppnet_dropout_ratio: [0.1, 0.2, 0.3]\n"))
    with pytest.raises(ValueError, match="task_domain_num"):
        _model(dev, text=TEXT.replace("task_domain_num: 2", "task_domain_num: 0"))
    with pytest.raises(ValueError, match="domain_input_name"):
        _model(dev, text=TEXT.replace('domain_input_name: "dom"', 'domain_input_name: "pid"'))
    with pytest.raises(ValueError, match="num_expert"):
        _model(dev, text=TEXT.replace(HIDDEN, HIDDEN + "        num_expert: 3\n"))
    _model(dev, text=TEXT.replace(HIDDEN, HIDDEN + "        ppnet_dropout_ratio: [0.1]\n"))  # (one ratio for every layer: fine)


def _train(dev, fused, monkeypatch, steps=3):
    monkeypatch.setattr(personalized_net, "FUSED_GATE_SCALE", fused)
    spec, model = _model(dev, seed=3)
    opt = FusedDenseAdam(list(model.dense_parameters()), lr=0.01)
    batch = next(synthetic_batches(spec, 96, 96, seed=4)).to(dev)
    losses = []
    for _ in range(steps):
        loss = model.loss(model(batch), batch)
        total = loss["binary_cross_entropy_ctr"] + loss["binary_cross_entropy_cvr"]
        opt.zero_grad()
        total.backward()
        opt.step()
        losses.append([float(v.detach()) for v in (loss["binary_cross_entropy_ctr"], loss["binary_cross_entropy_cvr"])])
    with torch.no_grad():
        out = model(batch)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters() if not n.startswith("embedding_group.")}
    tables = {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()}
    return torch.tensor(losses, dtype=torch.float64), [out[k].cpu() for k in sorted(out) if k.startswith("logits")], params, tables


def test_fused_and_literal_training_agree(dev, monkeypatch, fwd_calls):
    """three steps on one batch (Adam on the dense parameters, the fused sparse update inside backward) from one seed: the loss of
    every step and the logits of all four towers after the steps agree between the fused and the literal form within the module
    test's bound -- 4 x the reference's own fp32-vs-float64 distance stored with the module vectors (the largest of its kinds),
    floor 2^-20, relative to max(1, |value|).  The parameters and tables are printed, not held to it (tests/test_ple_config.py
    says why: an element's first Adam / Adagrad update is lr * g / (|g| + eps))."""
    calls = fwd_calls()
    la, ya, pa, ta = _train(dev, True, monkeypatch)
    n_fused = calls["n"]
    lb, yb, pb, tb = _train(dev, False, monkeypatch)
    assert n_fused == 4 * 3 and calls["n"] == n_fused  # EPNet + two levels per forward; the literal run never calls the kernel
    print("losses fused", la.tolist(), "literal", lb.tolist())
    vec = np.load(os.path.join(GOLDEN, "reference_pepnet_vectors.npz"))
    bound = max(4.0 * max(float(vec[k]) for k in vec.files if k.startswith("ref_gap/")), FLOOR)
    err_l, err_y = rel_err([la], [lb]), rel_err(ya, [y.double() for y in yb])
    err_p = max(rel_err([pa[n]], [pb[n].double()]) for n in pa)
    err_t = max(rel_err([ta[n]], [tb[n].double()]) for n in ta)
    print(f"fused vs literal after 3 steps on {dev.type}: losses {err_l:.3e} logits {err_y:.3e} bound {bound:.3e}; parameters {err_p:.3e} tables {err_t:.3e}")
    assert err_l <= bound and err_y <= bound


def _bce(x, y):
    return torch.nn.functional.binary_cross_entropy_with_logits(x, y, reduction="none")


def test_the_loss_reads_the_selected_domain(dev):
    spec, model = _model(dev, seed=5)
    batch = next(synthetic_batches(spec, 96, 96, seed=6))
    dom, clk, buy = (batch.labels[k].double() for k in ("dom", "clk", "buy"))
    assert 0 < int(dom.sum()) < 96
    batch = batch.to(dev)
    out = model(batch)
    loss = model.loss(out, batch)
    pick = lambda tower: torch.where(dom > 0, out[f"logits_{tower}_1"].detach().cpu().double(), out[f"logits_{tower}_0"].detach().cpu().double())  # noqa: E731
    w = torch.where(clk > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.5, dtype=torch.float64))  # cvr: out_task_space_weight 0.5
    want = {"binary_cross_entropy_ctr": _bce(pick("ctr"), clk).mean(), "binary_cross_entropy_cvr": (w * _bce(pick("cvr"), buy)).sum() / w.sum()}
    for k, v in want.items():
        print(f"{k} on {dev.type}: got {float(loss[k].detach()):.8f} want {float(v):.8f}")
        torch.testing.assert_close(loss[k].detach().cpu().double(), v, rtol=1e-5, atol=1e-6)


def test_unselected_domain_towers_get_exactly_zero_gradient(dev):
    spec, model = _model(dev, seed=7)
    batch = next(synthetic_batches(spec, 64, 64, seed=8))
    batch.labels["dom"] = torch.zeros_like(batch.labels["dom"])  # every sample of domain 0
    batch = batch.to(dev)
    loss = model.loss(model(batch), batch)
    (loss["binary_cross_entropy_ctr"] + loss["binary_cross_entropy_cvr"]).backward()
    for k in range(4):  # tower k = task * 2 + domain
        grads = [p.grad for p in list(model.task_mlps[k].parameters()) + list(model.task_outputs[k].parameters())]
        assert all(g is not None for g in grads)
        if k % 2 == 1:
            assert all(float(g.abs().max()) == 0.0 for g in grads), k
        else:
            assert all(float(g.abs().max()) > 0.0 for g in grads), k


def test_a_domain_id_out_of_range_selects_nothing():
    """CPU tensors only: the selection is a mask-and-sum, so a row whose id is outside [0, D) gets 0 for every kind and passes no
    gradient to any tower -- as ConfigPEPNet's docstring says -- where the reference's gather would fault"""
    spec = load_pipeline_spec(TEXT)
    model = build_rank_model(spec, device=torch.device("cpu"))
    ids = torch.tensor([0, 1, 2, -1, 1, 7], dtype=torch.int64)
    preds = {f"{kind}_{tower}_{d}": torch.randn(6, generator=torch.Generator().manual_seed(d + 10 * i)).requires_grad_(True)
             for i, (kind, tower) in enumerate((k, t) for k in ("logits", "probs") for t in ("ctr", "cvr")) for d in (0, 1)}
    sel = model.select_domain_predictions(preds, types.SimpleNamespace(labels={"dom": ids}))
    assert sorted(sel) == ["logits_ctr", "logits_cvr", "probs_ctr", "probs_cvr"]
    for key, v in sel.items():
        want = torch.stack([preds[key + "_0"][0], preds[key + "_1"][1], torch.tensor(0.0), torch.tensor(0.0), preds[key + "_1"][4], torch.tensor(0.0)])
        assert torch.equal(v.detach(), want.detach()), key
    sum(v.sum() for v in sel.values()).backward()
    for key, p in preds.items():
        d = int(key[-1])
        assert torch.equal(p.grad, (ids == d).float()), key


def test_dropout_is_applied_where_the_reference_applies_it(dev, fwd_calls):
    calls = fwd_calls()
    text = TEXT.replace(HIDDEN, HIDDEN + "        ppnet_dropout_ratio: [0.5]\n")
    spec, plain = _model(dev, seed=9)
    _, model = _model(dev, seed=9, text=text)
    assert [d.p for d in model.ppnet.dropout_ratios] == [0.5] * 4 and [d.p for d in plain.ppnet.dropout_ratios] == [0.0] * 4
    batch = next(synthetic_batches(spec, 50, 50, seed=10)).to(dev)
    with torch.no_grad():
        a, b = plain.eval()(batch), model.eval()(batch)
    assert all(torch.equal(a[k], b[k]) for k in a)  # eval(): the model without dropout
    model.train()
    out = model(batch)
    assert calls["n"] == 3 * 3  # (the kernel runs under dropout too: nn.Dropout on its output)
    loss = model.loss(out, batch)
    (loss["binary_cross_entropy_ctr"] + loss["binary_cross_entropy_cvr"]).backward()
    assert all(bool(torch.isfinite(v).all()) for v in out.values()) and not all(torch.equal(out[k].detach(), a[k]) for k in a)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.dense_parameters())


def test_evaluator_reads_the_selected_probabilities(dev):
    spec, model = _model(dev, seed=11)
    batches = list(synthetic_batches(spec, 2 * 64 + 5, 64, seed=12))
    got = evaluate(model, iter(batches), Evaluator(model, spec, dev))
    assert sorted(got) == ["auc_ctr", "auc_cvr"]
    mine = {"ctr": BinnedAUC(200, device=dev), "cvr": BinnedAUC(200, device=dev)}
    model.eval()
    with torch.no_grad():
        for hb in batches:
            b = hb.to(dev)
            out = model(b)
            for tower, label in (("ctr", "clk"), ("cvr", "buy")):
                probs = torch.where(b.labels["dom"] > 0, out[f"probs_{tower}_1"], out[f"probs_{tower}_0"])
                metric_update(probs, b.labels[label], auc=mine[tower])
    for tower in ("ctr", "cvr"):
        print(f"auc_{tower} on {dev.type}: evaluate {float(got[f'auc_{tower}']):.6f} from the selected probabilities {float(mine[tower].compute()):.6f}")
        assert float(got[f"auc_{tower}"]) == float(mine[tower].compute()) and 0.0 <= float(got[f"auc_{tower}"]) <= 1.0
