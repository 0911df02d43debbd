"""`train_config.dense_optimizer` -> the optimizer the reference would build (tzrec/optim/optimizer_builder.py:100-260):
every kind of the oneof with every field, `part_optimizers` grouped by regex with their own schedules -- config.py's
`dense_optimizer_from_config`, dense_optim's `build_dense_optimizer` / `create_dense_schedulers`."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from dense_optim_ref import Reference, check_bound  # noqa: E402
from torcheasyrec_amd import lr_scheduler as lrs  # noqa: E402
from torcheasyrec_amd.config import dense_optimizer_from_config, load_pipeline_spec, parse_text_proto  # noqa: E402
from torcheasyrec_amd.dense_opt_kinds import DENSE_KINDS  # noqa: E402
from torcheasyrec_amd.dense_optim import build_dense_optimizer, create_dense_schedulers, named_dense_parameters  # noqa: E402

HERE = os.path.dirname(__file__)

BLOCKS = {
    "sgd": ("sgd_optimizer { lr: 0.1 momentum: 0.5 weight_decay: 0.01 dampening: 0.25 nesterov: false fused: true }",
            {"lr": 0.1, "momentum": 0.5, "weight_decay": 0.01, "dampening": 0.25, "nesterov": False}),
    "adagrad": ("adagrad_optimizer { lr: 0.2 weight_decay: 0.001 initial_accumulator_value: 0.1 eps: 1e-9 }",
                {"lr": 0.2, "weight_decay": 0.001, "initial_accumulator_value": 0.1, "eps": 1e-9}),
    "adam": ("adam_optimizer { lr: 0.003 beta1: 0.8 beta2: 0.99 weight_decay: 0.02 eps: 1e-7 amsgrad: false }",
             {"lr": 0.003, "beta1": 0.8, "beta2": 0.99, "weight_decay": 0.02, "eps": 1e-7}),
    "adamw": ("adamw_optimizer { lr: 0.004 beta1: 0.85 beta2: 0.98 weight_decay: 0.05 eps: 1e-6 }",
              {"lr": 0.004, "beta1": 0.85, "beta2": 0.98, "weight_decay": 0.05, "eps": 1e-6}),
    "adadelta": ("adadelta_optimizer { lr: 1.0 rho: 0.9 eps: 1e-5 weight_decay: 0.01 }", {"lr": 1.0, "rho": 0.9, "eps": 1e-5, "weight_decay": 0.01}),
    "rmsprop": ("rmsprop_optimizer { lr: 0.01 alpha: 0.9 eps: 1e-7 weight_decay: 0.03 }", {"lr": 0.01, "alpha": 0.9, "eps": 1e-7, "weight_decay": 0.03}),
}
# protos/optimizer.proto:159-208
PROTO_DEFAULTS = {
    "sgd": {"lr": 0.002, "momentum": 0.9, "weight_decay": 0.0, "dampening": 0.0, "nesterov": False},
    "adagrad": {"lr": 0.002, "weight_decay": 0.0, "initial_accumulator_value": 0.0, "eps": 1e-10},
    "adam": {"lr": 0.002, "beta1": 0.9, "beta2": 0.999, "weight_decay": 0.0, "eps": 1e-8},
    "adamw": {"lr": 0.002, "beta1": 0.9, "beta2": 0.999, "weight_decay": 0.0, "eps": 1e-8},
    "adadelta": {"lr": 0.002, "rho": 0.95, "eps": 1e-6, "weight_decay": 0.0},
    "rmsprop": {"lr": 0.002, "alpha": 0.99, "eps": 1e-8, "weight_decay": 0.0},
}


@pytest.mark.parametrize("kind", list(BLOCKS))
def test_each_block_parses_to_its_kind_and_fields(kind):
    text, want = BLOCKS[kind]
    cfg = dense_optimizer_from_config(parse_text_proto(text + " constant_learning_rate { }"))
    assert cfg.kind == kind and cfg.fields == want and cfg.parts == [] and cfg.regex_pattern is None
    assert all(type(cfg.fields[k]) is type(v) for k, v in want.items())
    empty = dense_optimizer_from_config(parse_text_proto(f"{kind}_optimizer {{ }}"))
    assert empty.kind == kind and empty.fields == PROTO_DEFAULTS[kind]
    assert set(DENSE_KINDS) == set(BLOCKS)


def test_amsgrad_and_unknown_members_raise():
    for kind in ("adam", "adamw"):
        with pytest.raises(ValueError, match="amsgrad"):
            dense_optimizer_from_config(parse_text_proto(f"{kind}_optimizer {{ lr: 0.1 amsgrad: true }}"))
    with pytest.raises(ValueError, match="Unknown optimizer: lion_optimizer"):
        dense_optimizer_from_config(parse_text_proto("lion_optimizer { lr: 0.1 }"))
    with pytest.raises(ValueError, match="Unknown optimizer"):
        dense_optimizer_from_config(parse_text_proto("constant_learning_rate { }"))
    with pytest.raises(ValueError, match="Unknown optimizer: lamb_optimizer"):  # a sparse kind is not a dense one
        dense_optimizer_from_config(parse_text_proto("adam_optimizer { lr: 0.1 } part_optimizers { lamb_optimizer { } regex_pattern: \".*\" }"))
    with pytest.raises(ValueError, match="centered"):  # a field the message does not have
        dense_optimizer_from_config(parse_text_proto("rmsprop_optimizer { lr: 0.1 centered: true }"))
    with pytest.raises(ValueError, match="nesterov"):
        dense_optimizer_from_config(parse_text_proto("sgd_optimizer { lr: 0.1 nesterov: true dampening: 0.5 }"))


def test_pipeline_spec_keeps_the_old_fields_and_gains_the_new_one():
    spec = load_pipeline_spec(open(os.path.join(HERE, "golden", "deepfm_mini.config")).read())
    assert spec.dense_lr == 0.001 and spec.dense_optimizer_block.has("adam_optimizer")
    assert spec.dense_optimizer.kind == "adam" and spec.dense_optimizer.fields == dict(PROTO_DEFAULTS["adam"], lr=0.001)


PARTS = """
adam_optimizer { lr: 0.01 beta2: 0.99 }
exponential_decay_learning_rate { decay_size: 1 decay_factor: 0.5 }
part_optimizers { sgd_optimizer { lr: 0.5 momentum: 0.0 } regex_pattern: "tower\\\\.0\\\\..*" manual_step_learning_rate { schedule_sizes: [2] learning_rates: [0.25] } }
part_optimizers { rmsprop_optimizer { lr: 0.1 } regex_pattern: "nothing_like_this.*" }
part_optimizers { adagrad_optimizer { lr: 0.2 } regex_pattern: "tower\\\\..*\\\\.bias" }
part_optimizers { adadelta_optimizer { lr: 1.0 } regex_pattern: "bias" }
"""


def _named():
    names = ["tower.0.weight", "tower.0.bias", "tower.1.weight", "tower.1.bias", "head.weight", "head.bias", "xbias"]
    return [(n, torch.nn.Parameter(torch.zeros(3))) for n in names]


def test_part_optimizers_group_by_fullmatch_first_pattern_wins():
    cfg = dense_optimizer_from_config(parse_text_proto(PARTS))
    assert [p.kind for p in cfg.parts] == ["sgd", "rmsprop", "adagrad", "adadelta"]
    assert cfg.parts[0].regex_pattern == r"tower\.0\..*"
    named = _named()
    opt = build_dense_optimizer(named, cfg)
    name_of = {id(p): n for n, p in named}
    got = [(g["kind"], g["part"], [name_of[id(p)] for p in g["params"]]) for g in opt.param_groups]
    assert got == [
        # what no pattern matched: the main block's.  "bias" is a FULL match: it takes neither head.bias nor xbias
        ("adam", None, ["tower.1.weight", "head.weight", "head.bias", "xbias"]),
        ("sgd", 0, ["tower.0.weight", "tower.0.bias"]),  # tower.0.bias: the first matching pattern wins over part 2's
        ("adagrad", 2, ["tower.1.bias"]),
    ]  # parts 1 and 3 match nothing: no group
    assert opt.param_groups[0]["betas"] == (0.9, 0.99) and opt.param_groups[0]["lr"] == 0.01
    assert opt.param_groups[1]["momentum"] == 0.0 and opt.param_groups[2]["initial_accumulator_value"] == 0.0
    # a dict of parameters is taken like the reference's
    assert [g["kind"] for g in build_dense_optimizer(dict(named), cfg).param_groups] == ["adam", "sgd", "adagrad"]


def test_a_part_is_scheduled_by_its_own_learning_rate_or_the_main_blocks():
    cfg = dense_optimizer_from_config(parse_text_proto(PARTS))
    opt = build_dense_optimizer(_named(), cfg)
    sch = create_dense_schedulers(opt, cfg)
    assert [type(s) for s in sch] == [lrs.ExponentialDecayLR, lrs.ManualStepLR, lrs.ExponentialDecayLR]
    assert all(len(s.optimizer.param_groups) == 1 for s in sch)  # each drives its group alone
    rates = []
    for _ in range(4):
        rates.append([g["lr"] for g in opt.param_groups])
        for s in sch:
            s.step()
    assert [r[0] for r in rates] == pytest.approx([0.01, 0.005, 0.0025, 0.00125])  # main: halves every step
    assert [r[1] for r in rates] == pytest.approx([0.5, 0.5, 0.5, 0.25])            # part 0: its own manual steps
    assert [r[2] for r in rates] == pytest.approx([0.2, 0.1, 0.05, 0.025])          # part 2: the main block's decay, on ITS base rate
    # a block without the oneof: constant
    plain = dense_optimizer_from_config(parse_text_proto("sgd_optimizer { lr: 0.1 }"))
    assert [type(s) for s in create_dense_schedulers(build_dense_optimizer(_named(), plain), plain)] == [lrs.ConstantLR]


class _Both:
    """the fused optimizer and a reference fed the gradients the model's backward produced"""

    def __init__(self, opt, refs):
        self.opt, self.refs = opt, refs

    def zero_grad(self, set_to_none=True):
        self.opt.zero_grad(set_to_none)

    def step(self):
        grads = [None if p.grad is None else p.grad.detach().cpu().clone() for p in self.opt.params]
        self.opt.step()
        for r in self.refs:
            r.step(grads)


def test_a_config_that_names_momentum_sgd_trains_with_momentum_sgd(dev):
    """fails without the feature: the same config used to yield Adam(lr) whatever it named"""
    from test_config_plumbing import _batches
    from torcheasyrec_amd.embedding_group import TrainPipeline
    from torcheasyrec_amd.rank_model import build_rank_model

    text = open(os.path.join(HERE, "golden", "deepfm_mini.config")).read()
    old = text[text.index("adam_optimizer {"):text.index("}", text.index("adam_optimizer {")) + 1]
    text = text.replace(old, "sgd_optimizer { lr: 0.1 momentum: 0.5 }", 1)
    spec = load_pipeline_spec(text)
    assert spec.dense_optimizer.kind == "sgd" and spec.dense_lr == 0.1
    torch.manual_seed(0)
    model = build_rank_model(spec, device=dev)
    named = named_dense_parameters(model)
    assert len(named) == len(list(model.dense_parameters())) > 0
    opt = build_dense_optimizer(named, spec.dense_optimizer)
    assert [g["kind"] for g in opt.param_groups] == ["sgd"] and opt.param_groups[0]["momentum"] == 0.5
    init = [p.detach().cpu().clone() for p in opt.params]
    f32 = Reference("sgd", init, torch.float32, lr=0.1, momentum=0.5)
    f64 = Reference("sgd", init, torch.float64, lr=0.1, momentum=0.5)
    pipe = TrainPipeline(model, _Both(opt, [f32, f64]), dev, model.loss)
    it = iter(_batches(spec, 3 * spec.batch_size, spec.batch_size))
    for _ in range(3):
        pipe.progress(it)
    assert any(not torch.equal(p.detach().cpu(), q) for p, q in zip(opt.params, init))
    check_bound([p.detach() for p in opt.params], f32.values(), f64.values(), f"deepfm_mini with sgd_optimizer on {dev.type}")
    # (Adam's first steps move every element by about lr = 0.1: far outside this bound)
