"""The evaluation metrics of torcheasyrec_amd.metrics (csrc/eval_metrics.hip) against tests/metrics_ref.py and the reference's
own test literals (tests/golden/reference_metric_cases.json): on the lane emulator here, on the gfx950 library under `-m gpu`.

Tolerances: counts are integers (equality).  The AUC is a float64 trapezoid over identical integers on both sides (rtol
1e-12).  NE: the reference test's own atol 1e-6 on its literals; rtol 1e-5 against the float64 restatement (device logf /
log1pf against host log, a couple of fp32 ulps per term).  Grouped AUC: the integer 2U divided once, rtol 1e-12.

The last section runs batches above the kernels' grid caps (restated there and checked against the source), where a lane's
grid-stride loop and the block scan's top level take a second trip: the histogram is then compared with a binary-search
restatement (metrics_ref.bins_sorted, itself checked against the [B, T] comparison at small B)."""
import json
import os

import pytest
import torch

import metrics_ref as ref
from torcheasyrec_amd import _lib
from torcheasyrec_amd.metrics import BinnedAUC, GroupedAUC, NormalizedEntropy, metric_update

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_metric_cases.json")))
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _preds(B: int, T: int, seed: int) -> torch.Tensor:
    """0.0, 1.0, every threshold value, the floats just below and above a few thresholds, heavy ties, random values -- shuffled, and
    cut to B (B = 8199 holds all of them at every T used)"""
    g = torch.Generator().manual_seed(seed)
    thr = torch.linspace(0, 1, T)
    some = thr[:: max(T // 7, 1)]
    special = torch.cat([torch.tensor([0.0, 1.0]), thr, torch.nextafter(some, torch.tensor(-1.0)).clamp(min=0.0),
                         torch.nextafter(some, torch.tensor(2.0)).clamp(max=1.0), torch.full((max(B // 4, 1),), 0.5),
                         torch.full((max(B // 8, 1),), float(thr[T // 2]))])
    special = special[torch.randperm(special.numel(), generator=g)]
    if special.numel() >= B:
        return special[:B].clone()
    out = torch.cat([special, torch.rand(B - special.numel(), generator=g)])
    return out[torch.randperm(B, generator=g)]


def _labels(B: int, mode: str, seed: int) -> torch.Tensor:
    if mode == "mixed":
        return (torch.rand(B, generator=torch.Generator().manual_seed(seed + 1)) < 0.3).to(torch.int64)
    return torch.full((B,), 1 if mode == "ones" else 0, dtype=torch.int64)


@pytest.mark.parametrize("labels", ["zeros", "ones", "mixed"])
@pytest.mark.parametrize("T", [2, 200, 1000])
@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 1000, 8199])
def test_histogram_and_confusion_matrix_are_the_restatements_integers(dev, B, T, labels):
    p, y = _preds(B, T, seed=B * 31 + T), _labels(B, labels, seed=B + T)
    whole, parts = BinnedAUC(T, device=dev), BinnedAUC(T, device=dev)
    thr = whole.thresholds.cpu()
    assert torch.equal(thr, torch.linspace(0, 1, T))
    whole.update(p.to(dev), y.to(dev))
    # the same samples in three updates whose slices start at odd offsets (the kernel's unaligned form) accumulate to the same
    cuts = [0, B // 3 | 1 if B > 3 else 0, (2 * B // 3) | 1 if B > 3 else 0, B]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        parts.update(p[lo:hi].to(dev), y[lo:hi].to(dev))
    _sync(dev)
    want_hist, want_conf = ref.histogram(p, y, thr), ref.confmat(p, y, thr)
    for m in (whole, parts):
        assert torch.equal(m.histogram().cpu(), want_hist)
        assert m.confmat().dtype == torch.int64 and torch.equal(m.confmat().cpu(), want_conf)
    got, want = whole.compute().cpu(), ref.auc_from_confmat(want_conf)
    assert got.dtype == torch.float64 and not torch.isnan(got)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0.0)
    if labels != "mixed" or B == 0:
        assert got.item() == 0.0  # one class only: 0, not NaN
    whole.reset()
    assert int(whole.histogram().sum()) == 0


def test_binning_follows_the_comparison_at_every_threshold_edge(dev):
    """p >= thr[t] <=> bin(p) > t for the thresholds themselves and their neighbouring floats (p * (T - 1) arithmetic gets
    several of these wrong)"""
    T = 200
    m = BinnedAUC(T, device=dev)
    thr = m.thresholds.cpu()
    p = torch.cat([thr, torch.nextafter(thr, torch.tensor(-1.0)), torch.nextafter(thr, torch.tensor(2.0)), torch.tensor([float("nan"), -0.0, 1.5, -3.0])])
    y = torch.ones(p.numel(), dtype=torch.int64)
    m.update(p.to(dev), y.to(dev))
    _sync(dev)
    assert torch.equal(m.histogram().cpu(), ref.histogram(p, y, thr))


@pytest.mark.parametrize("case", GOLDEN["normalized_entropy"]["cases"], ids=lambda c: c["name"])
def test_normalized_entropy_reference_literals(dev, case):
    p, y = torch.tensor(case["preds"], dtype=torch.float32), torch.tensor(case["target"], dtype=torch.int64)
    want = torch.tensor(case["expected"], dtype=torch.float32)
    single, split = NormalizedEntropy(device=dev), NormalizedEntropy(device=dev)
    single.update(p.to(dev), y.to(dev))
    mid = p.numel() // 2
    split.update(p[:mid].to(dev), y[:mid].to(dev))
    split.update(p[mid:].to(dev), y[mid:].to(dev))
    for m in (single, split):
        torch.testing.assert_close(m.compute().cpu(), want, atol=GOLDEN["normalized_entropy"]["atol"], rtol=0)


@pytest.mark.parametrize("B", [1, 65, 1000, 8199])
def test_normalized_entropy_against_float64(dev, B):
    g = torch.Generator().manual_seed(B)
    p = torch.rand(B, generator=g)
    y = (torch.rand(B, generator=g) < 0.3).to(torch.int64)
    if B >= 65:  # p = 0 and p = 1 with both labels: the -100 clamp
        p[:4] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        y[:4] = torch.tensor([0, 1, 0, 1])
    else:
        y[0] = 1
    m = NormalizedEntropy(device=dev)
    m.update(p.to(dev), y.to(dev))
    _sync(dev)
    state = m.state().cpu()
    assert state[1].item() == B and state[2].item() == int(y.sum())
    want = ref.normalized_entropy(p, y)
    got = m.compute().cpu().to(torch.float64)
    print(f"NE B={B}: got {got.item():.9g} want {want.item():.9g} rel {abs(got.item() - want.item()) / abs(want.item()):.3g}")
    torch.testing.assert_close(got, want, rtol=1e-5, atol=0.0)


def test_degenerate_labels_and_boundary_predictions_stay_finite(dev):
    for label in (0, 1):
        m = NormalizedEntropy(device=dev)
        m.update(torch.full((128,), 0.3).to(dev), torch.full((128,), label, dtype=torch.int64).to(dev))
        assert torch.isfinite(m.compute()).item()
    m = NormalizedEntropy(device=dev)
    m.update(torch.tensor([0.0, 1.0, 1.0, 0.0]).to(dev), torch.tensor([0, 1, 0, 1]).to(dev))
    _sync(dev)
    assert m.state().cpu()[0].item() == 200.0  # two samples at the clamp, two at 0
    assert torch.isfinite(m.compute()).item()


def test_one_launch_updates_both_states(dev):
    p, y = _preds(1000, 200, 3), _labels(1000, "mixed", 3)
    auc, ne = BinnedAUC(200, device=dev), NormalizedEntropy(device=dev)
    calls = []
    L = _lib.lib()
    orig = L.tzr_metric_update
    L.tzr_metric_update = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        metric_update(p.to(dev), y.to(dev), auc=auc, ne=ne)
    finally:
        L.tzr_metric_update = orig
    _sync(dev)
    assert len(calls) == 1
    assert torch.equal(auc.confmat().cpu(), ref.confmat(p, y, auc.thresholds.cpu()))
    torch.testing.assert_close(ne.compute().cpu().to(torch.float64), ref.normalized_entropy(p, y), rtol=1e-5, atol=0.0)


def test_grouped_auc_reference_literal(dev):
    c = GOLDEN["grouped_auc"]
    m = GroupedAUC(capacity=16, device=dev)
    m.update(torch.tensor(c["preds"]).to(dev), torch.tensor(c["target"]).to(dev), torch.tensor(c["group_id"]).to(dev))
    assert m.compute().item() == c["expected"] == 0.5


def _grouped_rows(seed: int):
    """groups of 1, 2, 64, 65 and 5000 rows, negative keys and keys above 2^32, single-class groups among them, one group with
    every prediction tied, predictions from a small set of values (ties inside every group)"""
    g = torch.Generator().manual_seed(seed)
    sizes = [1, 1, 2, 2, 2, 64, 64, 65, 65, 5000, 3, 7, 100]
    keys_of = [-5, 7, -(1 << 40), (1 << 33) + 1, 3, 11, -1, (1 << 32), 12, (1 << 62), 0, 5, 6]
    keys = torch.cat([torch.full((n,), k, dtype=torch.int64) for n, k in zip(sizes, keys_of)])
    n = keys.numel()
    p = torch.randint(0, 50, (n,), generator=g).to(torch.float32) / 49.0
    y = (torch.rand(n, generator=g) < 0.4).to(torch.int64)
    y[keys == 3] = 1                      # a single-class group of two
    y[keys == 12] = 0                     # a single-class group of 65
    p[keys == 6] = 0.25                   # every prediction tied: AUC 0.5
    y[keys == 6] = (torch.arange(100) % 2)
    perm = torch.randperm(n, generator=g)
    return p[perm], y[perm], keys[perm]


@pytest.mark.parametrize("chunks", [1, 3])
def test_grouped_auc_against_pairwise_restatement(dev, chunks):
    p, y, k = _grouped_rows(5)
    n = p.numel()
    m = GroupedAUC(capacity=n + 10, device=dev)
    cuts = [n * i // chunks for i in range(chunks + 1)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m.update(p[lo:hi].to(dev), y[lo:hi].to(dev), k[lo:hi].to(dev))
    rp, ry, rk, overflow = m.rows()
    assert overflow == 0 and torch.equal(rp.cpu(), p) and torch.equal(ry.cpu().to(torch.int64), y) and torch.equal(rk.cpu(), k)
    want_sum, want_groups = ref.grouped_auc_parts(p, y, k)
    parts = GroupedAUC.reduce_rows(rp, ry, rk).cpu()
    assert int(parts[1]) == want_groups and want_groups >= 6
    torch.testing.assert_close(parts[0], torch.tensor(want_sum, dtype=torch.float64), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(m.compute().cpu(), torch.tensor(want_sum / want_groups, dtype=torch.float64), rtol=1e-12, atol=0.0)


def test_grouped_auc_all_tied_and_empty(dev):
    m = GroupedAUC(capacity=200, device=dev)
    m.update(torch.full((130,), 0.7).to(dev), (torch.arange(130) % 3 == 0).to(torch.int64).to(dev), torch.zeros(130, dtype=torch.int64).to(dev))
    assert m.compute().item() == 0.5
    m.reset()
    parts = GroupedAUC.reduce_rows(*m.rows()[:3]).cpu()
    assert parts.tolist() == [0.0, 0.0]


def test_grouped_auc_overflow_raises_and_keeps_the_rows_that_fit(dev):
    p, y, k = _grouped_rows(9)
    cap = 300
    m = GroupedAUC(capacity=cap, device=dev)
    m.update(p[:200].to(dev), y[:200].to(dev), k[:200].to(dev))
    m.update(p[200:500].to(dev), y[200:500].to(dev), k[200:500].to(dev))  # 100 fit, 200 do not
    m.update(p[500:520].to(dev), y[500:520].to(dev), k[500:520].to(dev))  # none fits
    rp, ry, rk, overflow = m.rows()
    assert overflow == 220 and rp.numel() == cap
    assert torch.equal(rp.cpu(), p[:cap]) and torch.equal(ry.cpu().to(torch.int64), y[:cap]) and torch.equal(rk.cpu(), k[:cap])
    with pytest.raises(RuntimeError, match="220 rows did not fit"):
        m.compute()


def test_abi_errors(dev):
    L, p = _lib.lib(), _lib.ptr
    probs, labels = torch.rand(8).to(dev), torch.ones(8, dtype=torch.int64).to(dev)
    thr = torch.linspace(0, 1, 5000).to(dev)
    hist = torch.zeros((5000 + 1) * 2, dtype=torch.int64).to(dev)
    ne = torch.zeros(3, dtype=torch.float64).to(dev)
    assert L.tzr_metric_update(p(probs), p(labels), 8, p(thr), 200, None, None, None) == INVALID           # no state at all
    assert L.tzr_metric_update(p(probs), p(labels), -1, p(thr), 200, p(hist), p(ne), None) == INVALID
    assert L.tzr_metric_update(p(probs), p(labels), 8, p(thr), 4097, p(hist), p(ne), None) == UNSUPPORTED  # above the LDS histogram
    assert L.tzr_metric_update(p(probs), p(labels), 8, None, 200, p(hist), None, None) == INVALID          # histogram without thresholds
    assert L.tzr_metric_update(p(probs), p(labels), 8, p(thr), 0, p(hist), None, None) == INVALID
    assert L.tzr_metric_update(None, p(labels), 8, p(thr), 200, p(hist), None, None) == INVALID
    assert L.tzr_metric_update(None, None, 0, p(thr), 200, p(hist), p(ne), None) == OK                      # B = 0: no-op
    assert L.tzr_metric_update(p(probs), p(labels), 8, None, 0, None, p(ne), None) == OK                    # NE alone
    assert L.tzr_metric_update(p(probs), p(labels), 8, p(thr), 4096, p(hist), None, None) == OK             # the cap itself
    _sync(dev)
    assert int(hist.sum()) == 8 and ne.cpu()[1].item() == 8.0
    rp, rl, rk = torch.zeros(4).to(dev), torch.zeros(4, dtype=torch.int32).to(dev), torch.zeros(4, dtype=torch.int64).to(dev)
    state = torch.zeros(4, dtype=torch.int64).to(dev)
    keys = torch.arange(8).to(dev)
    assert L.tzr_grouped_auc_append(p(probs), p(labels), p(keys), 8, p(rp), p(rl), p(rk), 4, None, None) == INVALID
    assert L.tzr_grouped_auc_append(p(probs), p(labels), p(keys), -1, p(rp), p(rl), p(rk), 4, p(state), None) == INVALID
    assert L.tzr_grouped_auc_append(p(probs), p(labels), None, 8, p(rp), p(rl), p(rk), 4, p(state), None) == INVALID
    assert L.tzr_grouped_auc_append(p(probs), p(labels), p(keys), 8, None, p(rl), p(rk), 4, p(state), None) == INVALID
    assert L.tzr_grouped_auc_append(None, None, None, 0, p(rp), p(rl), p(rk), 4, p(state), None) == OK
    assert L.tzr_grouped_auc_append(p(probs), p(labels), p(keys), 8, p(rp), p(rl), p(rk), 4, p(state), None) == OK
    _sync(dev)
    assert state.cpu().tolist() == [4, 4, 0, 0] and rk.cpu().tolist() == [0, 1, 2, 3]
    out, cnt = torch.zeros(1, dtype=torch.float64).to(dev), torch.zeros(1, dtype=torch.int64).to(dev)
    nbytes = L.tzr_grouped_auc_reduce_workspace(4)
    ws = _lib.workspace(nbytes, dev)
    assert L.tzr_grouped_auc_reduce_workspace(-1) == 0
    assert L.tzr_grouped_auc_reduce(p(rk), p(rp), p(rl), 4, None, p(cnt), p(ws), nbytes, None) == INVALID
    assert L.tzr_grouped_auc_reduce(p(rk), p(rp), p(rl), -1, p(out), p(cnt), p(ws), nbytes, None) == INVALID
    assert L.tzr_grouped_auc_reduce(None, p(rp), p(rl), 4, p(out), p(cnt), p(ws), nbytes, None) == INVALID
    assert L.tzr_grouped_auc_reduce(p(rk), p(rp), p(rl), 4, p(out), p(cnt), None, 0, None) == WORKSPACE
    assert L.tzr_grouped_auc_reduce(p(rk), p(rp), p(rl), 4, p(out), p(cnt), p(ws), nbytes - 1, None) == WORKSPACE
    assert L.tzr_grouped_auc_reduce(p(rk), p(rp), p(rl), 4, p(out), p(cnt), p(ws) + 8, nbytes, None) == WORKSPACE
    assert L.tzr_grouped_auc_reduce(p(rk), p(rp), p(rl), 4, p(out), p(cnt), p(ws), nbytes, None) == OK
    assert L.tzr_grouped_auc_reduce(None, None, None, 0, p(out), p(cnt), None, 0, None) == OK


# ---- past the grid caps: a lane's grid-stride loop runs twice, the block scan runs over more than 256 blocks --------------------
EM_THREADS, EM_VEC, EM_MAX_UPDATE_WGS, EM_MAX_APPEND_WGS = 256, 4, 512, 1024  # csrc/eval_metrics.hip
B_VEC = 524288 + 3079     # float4 form: above EM_MAX_UPDATE_WGS * EM_THREADS * EM_VEC, a whole-float4 tail and a scalar tail
B_SCALAR = 131072 + 1283  # scalar form: above EM_MAX_UPDATE_WGS * EM_THREADS
N_GROUPED = 300000


def test_the_big_updates_take_the_second_trip_of_every_capped_grid():
    src = open(os.path.join(os.path.dirname(__file__), "..", "torcheasyrec_amd", "csrc", "eval_metrics.hip")).read()
    for text in (f"#define EM_THREADS {EM_THREADS}", f"#define EM_VEC {EM_VEC} ", f"#define EM_MAX_UPDATE_WGS {EM_MAX_UPDATE_WGS}",
                 f"std::min<int64_t>({EM_MAX_APPEND_WGS}, (B + EM_THREADS - 1) / EM_THREADS)"):
        assert text in src, text  # the caps restated above are the kernels'
    assert B_VEC // EM_VEC > EM_MAX_UPDATE_WGS * EM_THREADS and B_VEC % EM_VEC != 0
    assert EM_MAX_UPDATE_WGS * EM_THREADS < B_SCALAR < EM_MAX_UPDATE_WGS * EM_THREADS * EM_VEC
    assert N_GROUPED > EM_MAX_APPEND_WGS * EM_THREADS                     # the append's loop
    assert -(-(N_GROUPED + 1) // EM_THREADS) > EM_THREADS                 # tzr_scan_top_kernel and the part_sum finish: a second trip


def test_the_searchsorted_restatement_bins_as_the_comparison_does():
    for T in (2, 200, 1000, 4096):
        thr = torch.linspace(0, 1, T)
        p = torch.cat([thr, torch.nextafter(thr, torch.tensor(-1.0)), torch.nextafter(thr, torch.tensor(2.0)),
                       torch.tensor([float("nan"), -0.0, 1.5, -3.0]), _preds(8199, T, seed=T)])
        assert torch.equal(ref.bins_sorted(p, thr), ref.bins(p, thr))


def _big_samples(B, T, seed):
    p, y = _preds(B, T, seed), _labels(B, "mixed", seed)
    p[:4], y[:4] = torch.tensor([0.0, 0.0, 1.0, 1.0]), torch.tensor([0, 1, 0, 1])  # the NE clamp, with both labels
    return p, y


def _misaligned(t, dev):
    """`t` on the device, 4 (float32) or 8 (int64) bytes behind a 16-byte boundary: the update's scalar form"""
    out = torch.cat([t[:1], t]).to(dev)[1:]
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def _aligned(t, dev):
    out = t.to(dev)
    assert out.data_ptr() % 16 == 0
    return out


@pytest.mark.parametrize("form,B,T", [("float4", B_VEC, 200), ("float4", B_VEC, 4096), ("scalar", B_SCALAR, 200)])
def test_metric_update_past_its_grid_cap(dev, form, B, T):
    p, y = _big_samples(B, T, seed=B + T)
    place = _aligned if form == "float4" else _misaligned
    auc, ne = BinnedAUC(T, device=dev), NormalizedEntropy(device=dev)
    metric_update(place(p, dev), place(y, dev), auc=auc, ne=ne)
    _sync(dev)
    assert torch.equal(auc.histogram().cpu(), ref.histogram(p, y, auc.thresholds.cpu(), ref.bins_sorted))
    state = ne.state().cpu()
    assert state[1].item() == B and state[2].item() == int(y.sum())
    want, got = ref.normalized_entropy(p, y), ne.compute().cpu().to(torch.float64)
    print(f"NE {form} B={B} on {dev.type}: got {got.item():.9g} want {want.item():.9g} rel {abs(got.item() - want.item()) / abs(want.item()):.3g}")
    torch.testing.assert_close(got, want, rtol=1e-5, atol=0.0)


def test_metric_updates_past_the_cap_accumulate(dev):
    """the same samples in one aligned update, and as an aligned update above the float4 form's cap followed by a misaligned
    one above the scalar form's"""
    T = 200
    p, y = _big_samples(B_VEC + B_SCALAR, T, seed=77)
    whole_auc, whole_ne = BinnedAUC(T, device=dev), NormalizedEntropy(device=dev)
    parts_auc, parts_ne = BinnedAUC(T, device=dev), NormalizedEntropy(device=dev)
    metric_update(_aligned(p, dev), _aligned(y, dev), auc=whole_auc, ne=whole_ne)
    metric_update(_aligned(p[:B_VEC], dev), _aligned(y[:B_VEC], dev), auc=parts_auc, ne=parts_ne)
    metric_update(_misaligned(p[B_VEC:], dev), _misaligned(y[B_VEC:], dev), auc=parts_auc, ne=parts_ne)
    _sync(dev)
    want = ref.histogram(p, y, whole_auc.thresholds.cpu(), ref.bins_sorted)
    assert torch.equal(whole_auc.histogram().cpu(), want) and torch.equal(parts_auc.histogram().cpu(), want)
    for ne in (whole_ne, parts_ne):
        state = ne.state().cpu()
        assert state[1].item() == p.numel() and state[2].item() == int(y.sum())
        torch.testing.assert_close(ne.compute().cpu().to(torch.float64), ref.normalized_entropy(p, y), rtol=1e-5, atol=0.0)
    torch.testing.assert_close(whole_auc.compute().cpu(), parts_auc.compute().cpu(), rtol=0.0, atol=0.0)


_BIG_GROUPED = {}


def _big_grouped_rows():
    """300 000 rows in about 9000 groups, one of them of about 12 000 rows; keys negative and above 2^40; predictions from 50
    values (ties inside every group); with the pairwise restatement's (sum, groups), computed once"""
    if not _BIG_GROUPED:
        g = torch.Generator().manual_seed(300)
        group = torch.cat([torch.zeros(12000, dtype=torch.int64), torch.randint(0, 9000, (N_GROUPED - 12000,), generator=g)])
        keys = torch.where(group % 2 == 0, group + (1 << 41), -group - 5)
        p = torch.randint(0, 50, (N_GROUPED,), generator=g).to(torch.float32) / 49.0
        y = (torch.rand(N_GROUPED, generator=g) < 0.4).to(torch.int64)
        perm = torch.randperm(N_GROUPED, generator=g)
        p, y, keys = p[perm], y[perm], keys[perm]
        assert int((keys == (1 << 41)).sum()) >= 12000 and bool((keys < 0).any()) and int(keys.max()) > (1 << 40)
        _BIG_GROUPED["rows"] = (p, y, keys)
        _BIG_GROUPED["want"] = ref.grouped_auc_parts(p, y, keys)
    return _BIG_GROUPED["rows"], _BIG_GROUPED["want"]


@pytest.mark.parametrize("chunks", [1, 3])
def test_grouped_auc_past_the_append_cap_and_one_scan_level(dev, chunks):
    (p, y, k), (want_sum, want_groups) = _big_grouped_rows()
    n = p.numel()
    m = GroupedAUC(capacity=n + 10, device=dev)
    cuts = [n * i // chunks for i in range(chunks + 1)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m.update(p[lo:hi].to(dev), y[lo:hi].to(dev), k[lo:hi].to(dev))
    rp, ry, rk, overflow = m.rows()
    assert overflow == 0 and torch.equal(rp.cpu(), p) and torch.equal(ry.cpu().to(torch.int64), y) and torch.equal(rk.cpu(), k)
    parts = GroupedAUC.reduce_rows(rp, ry, rk).cpu()
    assert int(parts[1]) == want_groups and want_groups > 8000
    torch.testing.assert_close(parts[0], torch.tensor(want_sum, dtype=torch.float64), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(m.compute().cpu(), torch.tensor(want_sum / want_groups, dtype=torch.float64), rtol=1e-12, atol=0.0)


def test_grouped_auc_overflow_in_the_second_trip_of_a_large_update(dev):
    (p, y, k), _ = _big_grouped_rows()
    n = p.numel()
    cap = n + EM_MAX_APPEND_WGS * EM_THREADS + 5000  # the second update's rows stop fitting inside its lanes' second trip
    assert n + EM_MAX_APPEND_WGS * EM_THREADS < cap < 2 * n
    m = GroupedAUC(capacity=cap, device=dev)
    m.update(p.to(dev), y.to(dev), k.to(dev))
    m.update(p.flip(0).to(dev), y.flip(0).to(dev), k.flip(0).to(dev))
    rp, ry, rk, overflow = m.rows()
    assert overflow == 2 * n - cap and rp.numel() == cap
    both = [torch.cat([t, t.flip(0)])[:cap] for t in (p, y, k)]
    assert torch.equal(rp.cpu(), both[0]) and torch.equal(ry.cpu().to(torch.int64), both[1]) and torch.equal(rk.cpu(), both[2])
    with pytest.raises(RuntimeError, match=f"{2 * n - cap} rows did not fit"):
        m.compute()
