"""tzr_dense_optim_fused (csrc/dense_optim_fused.hip) / dense_optim.FusedDenseOptimizer: the dense optimizer kinds a tzrec
config can name -- SGD, Adagrad, Adam, AdamW, Adadelta, RMSprop -- as groups of ONE launch, against torch.optim's
single-tensor path.  Bounds: Adam keeps the project's figure for this comparison (tests/test_dense_glue.py: rtol 2e-6,
atol 2e-7); the other kinds keep the derived bound of tests/dense_optim_ref.py."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from dense_optim_ref import Reference, check_bound, torch_optimizer  # noqa: E402
from torcheasyrec_amd import _lib, dense  # noqa: E402
from torcheasyrec_amd.dense_optim import FusedDenseOptimizer  # noqa: E402


@pytest.fixture(autouse=True)
def _reset_flag():
    dense.FUSE_FINISH = False
    dense._PENDING.clear()
    yield
    dense.FUSE_FINISH = False
    dense._PENDING.clear()


# (torch.optim.SGD refuses nesterov with dampening, so "nesterov" and "dampening" are two cases)
KINDS = {
    "sgd_plain": ("sgd", dict(lr=0.1, momentum=0.0)),
    "sgd_momentum": ("sgd", dict(lr=0.1, momentum=0.9)),
    "sgd_dampening": ("sgd", dict(lr=0.1, momentum=0.7, dampening=0.3)),
    "sgd_nesterov": ("sgd", dict(lr=0.05, momentum=0.8, nesterov=True)),
    "adagrad": ("adagrad", dict(lr=0.05, initial_accumulator_value=0.1, eps=1e-10)),
    "adam": ("adam", dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8)),
    "adamw": ("adamw", dict(lr=3e-3, betas=(0.8, 0.999), eps=1e-8)),
    "adadelta": ("adadelta", dict(lr=1.0, rho=0.9, eps=1e-6)),
    "rmsprop": ("rmsprop", dict(lr=1e-2, alpha=0.95, eps=1e-8)),
}
# one element | not a multiple of 256 | above 256 * 1024: the grid-stride loop runs | no gradient on some steps
SIZES = [1, 1000, 256 * 1024 + 300, 77]
SKIPPED = {3: (0, 3)}  # tensor 3 gets no gradient on steps 0 and 3: its first step is the run's second


def _grad(shape, step, i):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 * step + i))


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("case", list(KINDS))
def test_kind_matches_torch_optim(dev, case, weight_decay):
    kind, opts = KINDS[case]
    opts = dict(opts, weight_decay=weight_decay)
    torch.manual_seed(0)
    init = [torch.randn(n) for n in SIZES]
    ps = [torch.nn.Parameter(p.clone().to(dev)) for p in init]
    opt = FusedDenseOptimizer([{"kind": kind, "params": ps, **opts}])
    f64, f32 = Reference(kind, init, torch.float64, **opts), Reference(kind, init, torch.float32, **opts)
    steps = 8
    for step in range(steps):
        grads = [None if step in SKIPPED.get(i, ()) else _grad(p.shape, step, i) for i, p in enumerate(init)]
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.to(dev)
        opt.step()
        f64.step(grads)
        f32.step(grads)
    # step counts as torch counts them: per parameter, only on steps with a gradient; arrival counters back at zero
    assert opt._state[:, 0].cpu().tolist() == [float(steps - len(SKIPPED.get(i, ()))) for i in range(len(SIZES))]
    assert bool((opt._state[:, 1:] == 0).all())
    for i, r in enumerate(f32.params):
        if "step" in f32.opt.state[r]:
            assert float(f32.opt.state[r]["step"]) == float(opt._state[i, 0])
    check_bound([p.detach() for p in ps], f32.values(), f64.values(), f"{case} wd={weight_decay} on {dev.type}")
    if kind == "adam":
        for p, r in zip(ps, f32.params):
            torch.testing.assert_close(p.detach().cpu(), r.detach(), rtol=2e-6, atol=2e-7)


def _mixed(dev, n_tensors, seed=0):
    """three groups of different kinds and learning rates over n_tensors tensors -> (fused optimizer, its parameters per group,
    [(kind, opts, initial values)] per group)"""
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    specs = [("sgd", dict(lr=0.1, momentum=0.5, weight_decay=1e-3)), ("adamw", dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-2)),
             ("rmsprop", dict(lr=1e-3, alpha=0.9, eps=1e-8, weight_decay=0.0))]
    counts = [n_tensors - 2 * (n_tensors // 3), n_tensors // 3, n_tensors // 3]
    groups, per_group, refs = [], [], []
    for (kind, opts), c in zip(specs, counts):
        init = [torch.randn(int(n)) for n in rng.integers(1, 3000, size=c)]
        ps = [torch.nn.Parameter(p.clone().to(dev)) for p in init]
        groups.append({"kind": kind, "params": ps, **opts})
        per_group.append(ps)
        refs.append((kind, opts, init))
    return FusedDenseOptimizer(groups), per_group, refs


@pytest.fixture
def counted_entry(dev):
    """calls of the library's launch entry, counted as conftest.bwd_path counts its entries"""
    L = _lib.lib()
    orig = L.tzr_dense_optim_fused
    calls = {"n": 0, "tensors": []}

    def f(*a):
        calls["n"] += 1
        calls["tensors"].append(a[2])
        return orig(*a)

    L.tzr_dense_optim_fused = f
    try:
        yield calls
    finally:
        L.tzr_dense_optim_fused = orig


@pytest.mark.parametrize("n_tensors", [12, 40])
def test_mixed_groups_go_through_one_launch_per_32_tensors(dev, counted_entry, n_tensors):
    opt, per_group, refs = _mixed(dev, n_tensors)
    r64 = [Reference(k, init, torch.float64, **o) for k, o, init in refs]
    r32 = [Reference(k, init, torch.float32, **o) for k, o, init in refs]
    steps = 4
    for step in range(steps):
        at = 0
        for ps, a, b in zip(per_group, r64, r32):
            grads = [_grad(p.shape, step, at + i) for i, p in enumerate(ps)]
            at += len(ps)
            for p, g in zip(ps, grads):
                p.grad = g.to(dev)
            a.step(grads)
            b.step(grads)
        opt.step()
    # 12 tensors of three kinds: ONE call a step; 40: two (32 + 8), correct across the boundary
    assert counted_entry["n"] == steps * ((n_tensors + 31) // 32)
    assert counted_entry["tensors"][:2] == ([12] if n_tensors == 12 else [32, 8]) * (2 if n_tensors == 12 else 1)
    for gi, (ps, a, b) in enumerate(zip(per_group, r64, r32)):
        check_bound([p.detach() for p in ps], b.values(), a.values(), f"mixed group {gi} ({refs[gi][0]}) of {n_tensors} tensors on {dev.type}")


def _two_sgd_groups(dev):
    torch.manual_seed(3)
    init = [torch.randn(500), torch.randn(37)]
    a = [torch.nn.Parameter(p.clone().to(dev)) for p in init]
    b = [torch.nn.Parameter(p.clone().to(dev)) for p in init]
    opt = FusedDenseOptimizer([{"kind": "sgd", "lr": 0.1, "momentum": 0.5, "params": a}, {"kind": "rmsprop", "lr": 0.01, "params": b}])
    for i, p in enumerate(a + b):
        p.grad = _grad(p.shape, 0, i % 2).to(dev)
    return opt, a, b, init


def test_learning_rate_of_one_group_changes_only_that_group(dev):
    base, a0, b0, init = _two_sgd_groups(dev)
    opt, a1, b1, _ = _two_sgd_groups(dev)
    base.step()
    opt.step()
    opt.param_groups[1]["lr"] = 0.05
    base.step()
    opt.step()
    for p, q in zip(a0, a1):  # group 0: untouched by the other group's rate, bit for bit
        assert torch.equal(p.detach(), q.detach())
    for p, q in zip(b0, b1):
        assert not torch.equal(p.detach(), q.detach())
    ref = Reference("rmsprop", init, torch.float32, lr=0.01, alpha=0.99, eps=1e-8)
    ref64 = Reference("rmsprop", init, torch.float64, lr=0.01, alpha=0.99, eps=1e-8)
    for lr in (0.01, 0.05):
        for r in (ref, ref64):
            r.opt.param_groups[0]["lr"] = lr
            r.step([_grad(p.shape, 0, i) for i, p in enumerate(init)])
    check_bound([p.detach() for p in b1], ref.values(), ref64.values(), f"rmsprop group after its lr changed on {dev.type}")
    if dev.type != "cuda":
        return
    # the same through a captured graph: the kernel reads every group's rate from the device, sync_lr() moves it there
    cap, a2, b2, _ = _two_sgd_groups(dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap.step()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph.replay()
    cap.param_groups[1]["lr"] = 0.05
    cap.sync_lr()
    graph.replay()
    torch.cuda.synchronize(dev)
    for p, q in zip(a1 + b1, a2 + b2):
        assert torch.equal(p.detach(), q.detach())
    assert cap._state[:, 0].cpu().tolist() == [2.0] * 4


def test_state_dict_round_trip_is_bit_identical_and_names_are_torchs(dev):
    def run(split):
        opt, per_group, _ = _mixed(dev, 9, seed=5)
        ps = [p for g in per_group for p in g]
        for step in range(6):
            if split and step == 3:
                buf = io.BytesIO()
                torch.save(opt.state_dict(), buf)  # (as checkpoint.py saves and loads it)
                buf.seek(0)
                sd = torch.load(buf, weights_only=True)
                fresh, per_group2, _ = _mixed(dev, 9, seed=5)
                ps2 = [p for g in per_group2 for p in g]
                for p, q in zip(ps2, ps):
                    p.data.copy_(q.data)
                fresh._state[:, 1:] = 7.0  # (arrival counters are zeroed on load, whatever was there)
                fresh.load_state_dict(sd)
                assert bool((fresh._state[:, 1:] == 0).all())
                opt, ps = fresh, ps2
            for i, p in enumerate(ps):
                p.grad = _grad(p.shape, step, i).to(dev)
            opt.step()
        return [p.detach().cpu().clone() for p in ps], opt

    whole, _ = run(False)
    resumed, opt = run(True)
    for a, b in zip(whole, resumed):
        assert torch.equal(a, b)
    # the state names are torch.optim's
    sd = opt.state_dict()
    at = 0
    for g in sd["param_groups"]:
        kind = g["kind"]
        r = torch.nn.Parameter(torch.randn(3))
        topt = torch_optimizer(kind, [r], **{k: v for k, v in g.items() if k in ("lr", "momentum", "betas", "alpha", "eps", "weight_decay")})
        r.grad = torch.randn(3)
        topt.step()
        theirs = set(topt.state_dict()["state"][0]) - {"step"}
        for i in g["params"]:
            assert set(sd["state"][i]) - {"step"} == theirs, (kind, set(sd["state"][i]), theirs)
            assert float(sd["state"][i]["step"]) == 6.0
        assert g["params"] == list(range(at, at + len(g["params"])))
        at += len(g["params"])
    for kind, names in (("adagrad", {"sum"}), ("adam", {"exp_avg", "exp_avg_sq"}), ("adadelta", {"square_avg", "acc_delta"})):
        p = torch.nn.Parameter(torch.zeros(2, device=dev))
        assert set(FusedDenseOptimizer([{"kind": kind, "params": [p]}]).state_dict()["state"][0]) - {"step"} == names


def _train(dev, fuse, steps, counted, B=96):
    """the `_train` of tests/test_fused_adam.py with momentum SGD as the dense optimizer"""
    from torcheasyrec_amd.criteo import NUM_DENSE, SPARSE_KEYS, criteo_tables, synthetic_batch
    from torcheasyrec_amd.dlrm import DLRM
    from torcheasyrec_amd.embedding import SparseOptimizerConfig

    torch.manual_seed(0)
    rows = [min(r, 300) for r in [40000000, 39060, 17295, 7424, 20265, 3, 7122, 1543, 63, 40000000, 3067956, 405282, 10, 2209, 11938, 155, 4, 976, 14,
                                  40000000, 40000000, 40000000, 590152, 12973, 108, 36]]
    model = DLRM(criteo_tables(rows, init="seeded"), SPARSE_KEYS, NUM_DENSE, device=dev, sparse_optimizer=SparseOptimizerConfig(kind="sgd", lr=0.01))
    params = list(model.dense_parameters())
    dense.FUSE_FINISH = False
    opt = FusedDenseOptimizer([{"kind": "sgd", "lr": 1e-2, "momentum": 0.5, "weight_decay": 1e-3, "params": params}], fuse_finish=fuse)
    assert dense.FUSE_FINISH == fuse
    L = _lib.lib()
    orig = L.tzr_dense_optim_fused

    def f(*a):
        counted["partial"] += sum(1 for i in range(a[2]) if a[1][i].kind != _lib.ADAM_SRC_TENSOR)
        return orig(*a)

    L.tzr_dense_optim_fused = f
    try:
        for s in range(steps):
            d, kjt, y = synthetic_batch(s, B, rows)
            loss, _ = model.forward_loss(d.to(dev), kjt.to(dev), y.to(dev))
            with dense.root_loss():
                loss.backward(gradient=dense.unit_gradient(loss))
            opt.step()
            assert not dense._PENDING
            opt.zero_grad(set_to_none=True)
    finally:
        L.tzr_dense_optim_fused = orig
    return [p.detach().cpu().clone() for p in params], opt._state.cpu().clone(), float(loss.detach())


def test_momentum_sgd_with_gradients_left_as_partial_sums_is_bit_identical(dev):
    ca, cb = {"partial": 0}, {"partial": 0}
    pa, sa, la = _train(dev, False, 3, ca)
    pb, sb, lb = _train(dev, True, 3, cb)
    assert ca["partial"] == 0 and cb["partial"] > 0  # (the second run did take partial sums inside the optimizer's launch)
    assert la == lb
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    assert torch.equal(sa, sb) and bool((sa[:, 0] == 3).all()) and bool((sa[:, 1:] == 0).all())


def _abi_case(dev, n_good=1):
    """a table of `n_good` valid SGD tensors (param 1, grad 1, lr 0.5: a launch would move them to 0.5) and one Adam group"""
    ps = [torch.ones(8, device=dev) for _ in range(n_good + 1)]
    gs = [torch.ones(8, device=dev) for _ in range(n_good + 1)]
    st = torch.zeros(n_good + 1, 40, device=dev)
    m, v = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    tab = (_lib.TzrDenseOptTensor * (n_good + 1))()
    src = (_lib.TzrAdamSource * (n_good + 1))()
    for i in range(n_good + 1):
        tab[i].param, tab[i].grad, tab[i].state, tab[i].numel, tab[i].group = ps[i].data_ptr(), gs[i].data_ptr(), st[i].data_ptr(), 8, 0
    tab[n_good].group, tab[n_good].state0, tab[n_good].state1 = 1, m.data_ptr(), v.data_ptr()
    grp = (_lib.TzrDenseOptGroup * 9)()
    for j in range(9):
        grp[j].kind, grp[j].lr = 0, 0.5
    grp[1].kind, grp[1].hp0, grp[1].hp1, grp[1].eps = 2, 0.9, 0.999, 1e-8
    return ps, gs, st, (m, v), tab, src, grp


@pytest.mark.parametrize("case", ["groups", "kind", "state", "rows", "nowhere", "second_launch"])
def test_abi_refusals_return_an_error_and_launch_nothing(dev, case):
    L = _lib.lib()
    n_good = 34 if case == "second_launch" else 1  # (the bad tensor then sits in the SECOND launch of the call)
    ps, gs, st, mv, tab, src, grp = _abi_case(dev, n_good)
    n_groups, want, keep = 2, _lib.TZR_ERR_INVALID, None
    if case == "groups":
        n_groups, want = 9, _lib.TZR_ERR_UNSUPPORTED
    elif case == "kind":
        grp[1].kind = 99
    elif case in ("state", "second_launch"):
        tab[n_good].state1 = 0  # Adam needs two
    elif case == "rows":
        numel = 16 * 1024 + 1  # one workgroup more than the arrival counters of a state row hold
        keep = (torch.ones(numel, device=dev), torch.zeros(numel, device=dev), torch.zeros(numel, device=dev), torch.zeros(numel, device=dev))
        tab[n_good].param, tab[n_good].grad, tab[n_good].state0, tab[n_good].state1 = (t.data_ptr() for t in keep)
        tab[n_good].numel = numel
        src[n_good].kind, src[n_good].G, src[n_good].P, src[n_good].col, src[n_good].parts = _lib.ADAM_SRC_ROWS, 1, numel, 0, keep[1].data_ptr()
        want = _lib.TZR_ERR_UNSUPPORTED
    else:  # nowhere: partial sums to add up, neither a parameter to step nor a tensor to store them in
        parts = torch.ones(8, device=dev)
        keep = (parts,)
        tab[n_good].param, tab[n_good].grad = 0, 0
        src[n_good].kind, src[n_good].G, src[n_good].P, src[n_good].col, src[n_good].parts = _lib.ADAM_SRC_ROWS, 1, 8, 0, parts.data_ptr()
    rc = L.tzr_dense_optim_fused(tab, src, n_good + 1, grp, n_groups, None, _lib.stream_ptr(dev))
    assert rc == want
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    for p in ps:  # nothing was launched: not even the valid tensors in front of the bad one moved
        assert bool((p == 1).all())
    assert bool((st == 0).all())
    # ... and the same table without the fault steps them
    ps, gs, st, mv, tab, src, grp = _abi_case(dev, n_good)
    assert L.tzr_dense_optim_fused(tab, src, n_good + 1, grp, 2, None, _lib.stream_ptr(dev)) == _lib.TZR_OK
    for p in ps[:n_good]:
        assert bool((p == 0.5).all())
    assert st[:, 0].cpu().tolist() == [1.0] * (n_good + 1)
    del keep, gs, mv
