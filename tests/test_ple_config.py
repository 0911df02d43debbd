"""`ple {...}` from its config (tests/golden/ple_mini.config): the model the reference builds from the same file
(tzrec/models/ple.py:27-109), the gate-and-mix step of each CGC level on csrc/gate_mix.hip."""
import os

import numpy as np
import pytest
import torch

from cross_v2_ref import FLOOR, rel_err
from examples.train_from_config import synthetic_batches
from torcheasyrec_amd import _lib, ple
from torcheasyrec_amd.config import load_pipeline_spec
from torcheasyrec_amd.dense import FusedDenseAdam
from torcheasyrec_amd.metrics import Evaluator, evaluate
from torcheasyrec_amd.ple import ExtractionNet
from torcheasyrec_amd.rank_model import ConfigMMoE, ConfigPLE, MultiTaskRankModel, build_rank_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT = open(os.path.join(GOLDEN, "ple_mini.config")).read()
LEVEL1_SHARE = "            share_num: 1\n"
LEVEL1_SHARE_NET = "            share_expert_net { hidden_units: [24] }\n"


def _model(dev, seed=0, text=TEXT):
    spec = load_pipeline_spec(text)
    torch.manual_seed(seed)
    return spec, build_rank_model(spec, device=dev)


@pytest.fixture
def fwd_calls():
    calls = {"n": 0, "lib": None, "orig": None}

    def arm():
        L = _lib.lib()
        calls["lib"], calls["orig"] = L, L.tzr_cgc_mix_fwd

        def counted(*a):
            calls["n"] += 1
            return calls["orig"](*a)

        L.tzr_cgc_mix_fwd = counted
        return calls

    yield arm
    if calls["lib"] is not None:
        calls["lib"].tzr_cgc_mix_fwd = calls["orig"]


def test_config_builds_the_references_model(dev):
    spec, model = _model(dev)
    assert spec.model_name == "ple" and type(model) is ConfigPLE and isinstance(model, MultiTaskRankModel) and issubclass(ConfigMMoE, MultiTaskRankModel)
    assert model.embedding_group.group_total_dim("all") == 49
    l1, l2 = model._extraction_nets
    assert isinstance(l1, ExtractionNet) and not l1._final_flag and l2._final_flag and l1.name == "layer1" and l2.name == "layer2"
    assert l1.output_dim() == [24, 24, 24] and l2.output_dim() == [16, 16, 16]
    # level 1: two experts per task + one shared, three gates; level 2: one per task + two shared, no shared gate
    assert [len(t) for t in l1._task_layers] == [2, 2] and len(l1._shared_layers) == 1 and l1._shared_gate.weight.shape == (5, 49)
    assert [g.weight.shape for g in l1._task_gates] == [(3, 49), (3, 49)]
    assert [len(t) for t in l2._task_layers] == [1, 1] and len(l2._shared_layers) == 2 and l2._shared_gate is None
    assert [g.weight.shape for g in l2._task_gates] == [(3, 24), (3, 24)]
    assert l1._sels == [[0, 1, 4], [2, 3, 4], [0, 1, 2, 3, 4]] and l2._sels == [[0, 2, 3], [1, 2, 3]]
    keys = {k for k in model.state_dict() if not k.startswith("embedding_group.")}
    assert "_extraction_nets.0._shared_gate.weight" in keys and "_extraction_nets.1._task_layers.1.0.mlp.0.bias" in keys
    assert "_extraction_nets.1._shared_gate.weight" not in keys and "_extraction_nets.0._task_layers.0.1.mlp.2.weight" in keys
    assert {k.split(".")[0] for k in keys} == {"_extraction_nets", "task_mlps", "task_outputs"}
    assert len(list(model.dense_parameters())) == len(keys) == 52
    assert model.task_mlps[0].mlp[0].in_features == 16


def _recompose(features, model, dtype):
    """the towers' logits from the group's features and the model's own parameters in plain torch on the CPU: per level every
    expert (Linear + ReLU stacks), every gate as softmax(Linear) over the literal stack of its experts in the reference's order"""
    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items() if not k.startswith("embedding_group.")}
    lin = torch.nn.functional.linear

    def mlp(x, prefix):
        i = 0
        while f"{prefix}.mlp.{i}.weight" in sd:
            x = torch.relu(lin(x, sd[f"{prefix}.mlp.{i}.weight"], sd[f"{prefix}.mlp.{i}.bias"]))
            i += 2
        return x

    def gate(x, experts, prefix):
        w = torch.softmax(lin(x, sd[f"{prefix}.weight"], sd[f"{prefix}.bias"]), dim=1)
        return torch.matmul(w.unsqueeze(1), torch.stack(experts, dim=1)).squeeze(1)

    x = features.detach().cpu().to(dtype)
    task, shared = [x, x], x
    for lv, (P, S, final) in enumerate(((2, 1, False), (1, 2, True))):
        pre = f"_extraction_nets.{lv}"
        shared_experts = [mlp(shared, f"{pre}._shared_layers.{s}") for s in range(S)]
        all_task, outs = [], []
        for t in range(2):
            mine = [mlp(task[t], f"{pre}._task_layers.{t}.{j}") for j in range(P)]
            outs.append(gate(task[t], mine + shared_experts, f"{pre}._task_gates.{t}"))
            all_task += mine
        shared = None if final else gate(shared, all_task + shared_experts, f"{pre}._shared_gate")
        task = outs
    return [lin(mlp(task[t], f"task_mlps.{t}"), sd[f"task_outputs.{t}.weight"], sd[f"task_outputs.{t}.bias"]).squeeze(1) for t in range(2)]


@pytest.mark.parametrize("fused", [True, False])
def test_forward_is_the_plain_torch_restatement(dev, monkeypatch, fwd_calls, fused):
    monkeypatch.setattr(ple, "FUSED_CGC_MIX", fused)
    calls = fwd_calls()
    spec, model = _model(dev, seed=1)
    batch = next(synthetic_batches(spec, 100, 100, seed=2)).to(dev)
    with torch.no_grad():
        features = model.build_input(batch)["all"]
        out = model(batch)
    assert calls["n"] == (2 if fused else 0)  # one launch per level; FUSED_CGC_MIX = False never calls the kernel
    assert sorted(out) == ["logits_ctr", "logits_cvr", "probs_ctr", "probs_cvr"]
    got = [out["logits_ctr"], out["logits_cvr"]]
    want = _recompose(features, model, torch.float64)
    gap = rel_err(_recompose(features, model, torch.float32), want)
    err, bound = rel_err(got, want), max(4.0 * gap, FLOOR)
    print(f"logits on {dev.type} fused={fused}: err {err:.3e} literal fp32 gap {gap:.3e} bound {bound:.3e}")
    assert got[0].shape == (100,) and err <= bound
    torch.testing.assert_close(out["probs_cvr"], torch.sigmoid(out["logits_cvr"]))


def _train(dev, fused, monkeypatch, steps=4):
    monkeypatch.setattr(ple, "FUSED_CGC_MIX", fused)
    spec, model = _model(dev, seed=3)
    opt = FusedDenseAdam(list(model.dense_parameters()), lr=0.01)
    batch = next(synthetic_batches(spec, 96, 96, seed=4)).to(dev)
    losses = []
    for _ in range(steps):
        loss = model.loss(model(batch), batch)
        assert sorted(loss) == ["binary_cross_entropy_ctr", "binary_cross_entropy_cvr"]
        total = loss["binary_cross_entropy_ctr"] + loss["binary_cross_entropy_cvr"]
        opt.zero_grad()
        total.backward()
        opt.step()
        losses.append([float(v.detach()) for v in (loss["binary_cross_entropy_ctr"], loss["binary_cross_entropy_cvr"])])
    with torch.no_grad():
        out = model(batch)
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters() if not n.startswith("embedding_group.")}
    tables = {n: w.detach().cpu().clone() for n, w in model.embedding_group.ebc.table_weights().items()}
    return torch.tensor(losses, dtype=torch.float64), [out["logits_ctr"].cpu(), out["logits_cvr"].cpu()], params, tables


def test_training_lowers_the_loss_and_both_forms_agree(dev, monkeypatch, fwd_calls):
    """four steps on one batch (Adam on the dense parameters, the fused sparse update inside backward): both towers' losses
    fall, and what the fused and the literal form compute agrees within the module test's bound -- 4 x the reference's own
    fp32-vs-float64 distance stored with the module vectors (the largest of its kinds), floor 2^-20, relative to
    max(1, |value|) -- for the loss of every step and the logits of both towers after the steps.  The parameters and tables
    themselves are printed, not held to it: both optimizers divide by a running norm of the gradient (Adam's sqrt(v), the sparse
    Adagrad's sqrt(sum g^2), both starting at 0), so an element's first update is lr * g / (|g| + eps) and a rounding difference
    in a gradient near eps comes back multiplied by lr / (|g| + eps) whichever form computed it (measured on the emulator: tables
    1.3e-6 after ONE step and no more after four, dense parameters 4.2e-7)."""
    calls = fwd_calls()
    la, ya, pa, ta = _train(dev, True, monkeypatch)
    n_fused = calls["n"]
    lb, yb, pb, tb = _train(dev, False, monkeypatch)
    assert n_fused == 4 * 2 + 2 and calls["n"] == n_fused  # two levels per forward; the literal run never calls the kernel
    print("losses fused", la.tolist(), "literal", lb.tolist())
    assert bool((la[-1] < la[0]).all()) and bool((lb[-1] < lb[0]).all())
    vec = np.load(os.path.join(GOLDEN, "reference_ple_vectors.npz"))
    bound = max(4.0 * max(float(vec[k]) for k in vec.files if k.startswith("ref_gap/")), FLOOR)
    err_l, err_y = rel_err([la], [lb]), rel_err(ya, [y.double() for y in yb])
    err_p = max(rel_err([pa[n]], [pb[n].double()]) for n in pa)
    err_t = max(rel_err([ta[n]], [tb[n].double()]) for n in ta)
    print(f"fused vs literal after 4 steps on {dev.type}: losses {err_l:.3e} logits {err_y:.3e} bound {bound:.3e}; parameters {err_p:.3e} tables {err_t:.3e}")
    assert err_l <= bound and err_y <= bound


def test_evaluator_returns_the_per_tower_metrics(dev):
    spec, model = _model(dev, seed=5)
    got = evaluate(model, synthetic_batches(spec, 2 * 64 + 5, 64, seed=6), Evaluator(model, spec, dev))
    assert sorted(got) == ["auc_ctr", "auc_cvr"] and all(0.0 <= float(v) <= 1.0 for v in got.values())


def test_configs_the_reference_cannot_run_are_refused(dev):
    assert TEXT.count(LEVEL1_SHARE) == 1 and TEXT.count(LEVEL1_SHARE_NET) == 1
    with pytest.raises(ValueError, match="share_num"):
        _model(dev, text=TEXT.replace(LEVEL1_SHARE, ""))
    with pytest.raises(ValueError, match="share_num"):
        _model(dev, text=TEXT.replace(LEVEL1_SHARE, "            share_num: 0\n"))
    with pytest.raises(ValueError, match="share_expert_net"):
        _model(dev, text=TEXT.replace(LEVEL1_SHARE_NET, ""))
    with pytest.raises(ValueError, match="widths must be equal"):
        _model(dev, text=TEXT.replace(LEVEL1_SHARE_NET, "            share_expert_net { hidden_units: [20] }\n"))
    with pytest.raises(ValueError, match="num_expert"):
        _model(dev, text=TEXT.replace(LEVEL1_SHARE, LEVEL1_SHARE + "            num_expert: 3\n"))


def test_a_level_over_the_kernels_limits_takes_the_literal_form(dev, fwd_calls):
    """expert widths that are no multiple of 4: cgc_mix_ok refuses, the literal form runs, nothing raises"""
    calls = fwd_calls()
    text = TEXT.replace("hidden_units: [32, 24]", "hidden_units: [32, 22]").replace(LEVEL1_SHARE_NET, "            share_expert_net { hidden_units: [22] }\n")
    spec, model = _model(dev, text=text)
    batch = next(synthetic_batches(spec, 20, 20, seed=2)).to(dev)
    loss = model.loss(model(batch), batch)
    (loss["binary_cross_entropy_ctr"] + loss["binary_cross_entropy_cvr"]).backward()
    assert calls["n"] == 1  # level 2 (16 wide) still is one launch
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.dense_parameters())
