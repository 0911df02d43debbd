"""gate_ops.cgc_mix (tzr_cgc_mix_fwd / _bwd, csrc/gate_mix.hip): softmax + mixing of EVERY gate of one CGC level of PLE in one launch
per direction, each gate over its own subset of the experts, against the reference's stack / softmax / batched-matmul form
(tzrec/modules/extraction_net.py:98-109) evaluated in float64 on the CPU.  Tolerances: those of
tests/test_dense_glue.py::test_moe_mix_matches_the_stacked_form -- outputs and expert gradients rtol 1e-5, atol 1e-6; logit
gradients rtol 1e-4, atol 1e-5 * sqrt(H) (a sum of H products of O(1) terms in fp32)."""
import pytest
import torch

from torcheasyrec_amd import _lib


def ple_sels(T, P, S, final):
    """member lists of a CGC level over experts = [task 0's P | ... | task T-1's P | S shared]: task gate t its own then the
    shared ones, the shared gate (absent on the last level) every task expert in task order then the shared ones"""
    shared = list(range(T * P, T * P + S))
    sels = [list(range(t * P, (t + 1) * P)) + shared for t in range(T)]
    return sels if final else sels + [list(range(T * P)) + shared]


def literal64(logits, experts, sels, gouts):
    """the reference's form in float64: (outs, d_logits, d_experts); an expert of no gate gets zeros, a gate without an
    output gradient contributes nothing"""
    lg = [t.detach().cpu().double().clone().requires_grad_(True) for t in logits]
    xs = [t.detach().cpu().double().clone().requires_grad_(True) for t in experts]
    outs = [torch.matmul(torch.softmax(l, dim=1).unsqueeze(1), torch.stack([xs[e] for e in sel], dim=1)).squeeze(1) for l, sel in zip(lg, sels)]
    pairs = [(o, g.detach().cpu().double()) for o, g in zip(outs, gouts) if g is not None]
    grads = torch.autograd.grad([o for o, _ in pairs], lg + xs, [g for _, g in pairs], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, lg + xs)]
    return [o.detach() for o in outs], grads[:len(lg)], grads[len(lg):]


def draw(B, H, n_experts, sels, dev, seed, strided=False):
    """experts and output gradients ~ N(0,1), logits ~ 2 N(0,1); strided: column slices [:, 4 : 4 + H] of buffers 12 wider"""
    g = torch.Generator().manual_seed(seed)

    def rows():
        if strided:
            return torch.randn(B, H + 12, generator=g).to(dev)[:, 4:4 + H]
        return torch.randn(B, H, generator=g).to(dev)

    experts = [rows().requires_grad_(True) for _ in range(n_experts)]
    logits = [(2.0 * torch.randn(B, len(sel), generator=g)).to(dev).requires_grad_(True) for sel in sels]
    gouts = [rows() for _ in sels]
    return logits, experts, gouts


def run(logits, experts, sels, gouts):
    from torcheasyrec_amd.gate_ops import cgc_mix, cgc_mix_ok

    assert cgc_mix_ok(logits, experts, sels)
    outs = cgc_mix(logits, experts, sels)
    pairs = [(o, g) for o, g in zip(outs, gouts) if g is not None]
    grads = torch.autograd.grad([o for o, _ in pairs], logits + experts, [g for _, g in pairs], allow_unused=True)
    assert all(g is not None for g in grads)  # (one Function: every input gets a gradient, zeros where nothing flows)
    return [o.detach() for o in outs], list(grads[:len(logits)]), list(grads[len(logits):])


def check(got, want, H, what):
    for kind, rtol, atol in (("out", 1e-5, 1e-6), ("d_logits", 1e-4, 1e-5 * H ** 0.5), ("d_expert", 1e-5, 1e-6)):
        for i, (a, e) in enumerate(zip(got[kind], want[kind])):
            err = float((a.cpu().double() - e).abs().max()) if e.numel() else 0.0
            print(f"{what} {kind}[{i}]: max abs err {err:.3e} (max |want| {float(e.abs().max()):.3e})")
            torch.testing.assert_close(a.cpu().double(), e, rtol=rtol, atol=atol, msg=lambda m, k=kind, i=i: f"{what} {k}[{i}]: {m}")


def as_dict(t):
    return dict(zip(("out", "d_logits", "d_expert"), t))


# (B, H, T, P, S, final): one gate over one expert; three gates; the widest row group (64 lanes, four passes over its columns)
# on a last level; 12 experts under 5 gates with 66 float4 columns (a partial second pass per lane group); 16 experts, rows
# that are no multiple of the rows per wave or per workgroup; (4100, 256): 1025 workgroups' worth of rows, one more than the
# grid is capped at -- the row loop of some waves runs twice, of the others once
SHAPES = [(1, 4, 1, 0, 1, True), (37, 8, 2, 1, 1, False), (70, 1024, 1, 1, 1, True), (513, 264, 4, 2, 4, False), (4099, 64, 3, 4, 4, False),
          (4100, 256, 1, 1, 1, True)]
# experts and output gradients as strided column slices of wider buffers: at the four smaller shapes
CASES = [(*s, False) for s in SHAPES] + [(*s, True) for s in SHAPES[:4]]


@pytest.mark.parametrize("B,H,T,P,S,final,strided", CASES)
def test_cgc_mix_matches_the_stacked_form(dev, B, H, T, P, S, final, strided):
    sels = ple_sels(T, P, S, final)
    n_experts = T * P + S
    assert (len(sels), n_experts) in {(1, 1), (3, 3), (1, 2), (5, 12), (4, 16)}
    logits, experts, gouts = draw(B, H, n_experts, sels, dev, seed=B + H, strided=strided)
    if len(sels) > 1:
        gouts[1] = None  # one gate whose output gets no gradient
    got = as_dict(run(logits, experts, sels, gouts))
    check(got, as_dict(literal64(logits, experts, sels, gouts)), H, f"B{B} H{H}")
    again = as_dict(run(logits, experts, sels, gouts))
    for kind in got:
        assert all(torch.equal(a, b) for a, b in zip(got[kind], again[kind])), f"{kind}: two runs differ"


def test_cgc_mix_takes_any_membership(dev):
    """not PLE's pattern: expert 3 in exactly one gate, expert 1 in none (its gradient is zero, stored, not left unwritten),
    gate 1 lists its members out of order"""
    B, H, sels = 45, 20, [[2, 0], [4, 3, 0], [2]]
    logits, experts, gouts = draw(B, H, 5, sels, dev, seed=11)
    got = as_dict(run(logits, experts, sels, gouts))
    check(got, as_dict(literal64(logits, experts, sels, gouts)), H, "any membership")
    assert float(got["d_expert"][1].abs().max()) == 0.0 and float(got["d_expert"][3].abs().max()) > 0.0
    # a non-finite expert stays out of the gates that do not mix it
    with torch.no_grad():
        experts[3][0, 0] = float("nan")
    out = run(logits, experts, sels, gouts)[0]
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all()) and not bool(torch.isfinite(out[1]).all())


def test_cgc_mix_ok_refuses_what_the_kernel_does_not_take(dev):
    from torcheasyrec_amd.gate_ops import cgc_mix_ok

    def case(B=6, H=8, n_experts=3, n_gates=2, dtype=torch.float32):
        sels = [list(range(n_experts))] * n_gates
        return ([torch.zeros(B, n_experts, dtype=dtype, device=dev) for _ in sels], [torch.zeros(B, H, dtype=dtype, device=dev) for _ in range(n_experts)],
                sels)

    assert cgc_mix_ok(*case()) and cgc_mix_ok(*case(n_experts=16, n_gates=5)) and cgc_mix_ok(*case(H=4096))
    assert not cgc_mix_ok(*case(H=6)) and not cgc_mix_ok(*case(H=4100))
    assert not cgc_mix_ok(*case(n_experts=17)) and not cgc_mix_ok(*case(n_gates=6)) and not cgc_mix_ok(*case(dtype=torch.float16))
    assert not cgc_mix_ok(*case(B=0))
    lg, xs, _ = case()
    assert not cgc_mix_ok(lg, xs, [[0, 1, 1], [0, 1, 2]]) and not cgc_mix_ok(lg, xs, [[0, 1, 3], [0, 1, 2]])  # twice; out of range
    assert not cgc_mix_ok(lg, xs, [[0, 1], [0, 1, 2]])  # logits wider than the member list
    assert _lib.CGC_MAX_EXPERTS == 16 and _lib.CGC_MAX_GATES == 5


def run_abi(dev, xs, ls, gos, sels):
    """forward then backward at the C entry points on column slices of wider NaN-filled tensors, the layout of
    tests/test_dense_glue_kernels.py::run_moe; `sels` None: tzr_moe_mix_*, otherwise tzr_cgc_mix_* with these member lists"""
    import ctypes as C

    import test_dense_glue_kernels as glue

    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    (B, H), E, G = xs[0].shape, len(xs), len(ls)
    if sels is None:
        m, stem = _lib.TzrMoeMix(), "tzr_moe_mix"
        m.n_tasks = G
    else:
        m, stem = _lib.TzrCgcMix(), "tzr_cgc_mix"
        m.n_gates = G
        for g, sel in enumerate(sels):
            m.n_sel[g] = len(sel)
            for j, e in enumerate(sel):
                m.sel[g][j] = e
    m.B, m.H, m.n_experts = B, H, E
    keep, outs = [], {"out": [], "probs": [], "d_logits": [], "d_expert": []}
    for e, x in enumerate(xs):
        xw, xv = glue._wide(x, dev, 4 * (e % 3))
        dw, dv = glue._blank(B, H, dev, 4 * ((e + 1) % 3) + 12)
        m.expert[e], m.expert_stride[e], m.d_expert[e], m.d_expert_stride[e] = p(xv), xv.stride(0), p(dv), dv.stride(0)
        keep += [xw, (dw, dv)]
        outs["d_expert"].append(dv)
    for g in range(G):
        lw, lv = glue._cols(ls[g], dev, E + 3, 1)
        dlw, dlv = glue._cols((B, E), dev, E + 3, 1)
        ow, ov = glue._blank(B, H, dev, 4 * g + 24)
        gw, gv = glue._wide(gos[g], dev, 4 * g + 40)
        probs = torch.full((B, E), float("nan"), dtype=torch.float32, device=dev)
        m.logits[g], m.logits_stride[g], m.probs[g] = p(lv), lw.stride(0), p(probs)
        m.out[g], m.out_stride[g] = p(ov), ov.stride(0)
        m.grad_out[g], m.grad_out_stride[g] = p(gv), gv.stride(0)
        m.d_logits[g], m.d_logits_stride[g] = p(dlv), dlw.stride(0)
        keep += [lw, gw, (dlw, dlv), (ow, ov)]
        outs["out"].append(ov)
        outs["probs"].append(probs)
        outs["d_logits"].append(dlv)
    assert getattr(lib, stem + "_fwd")(C.byref(m), st) == 0
    assert getattr(lib, stem + "_bwd")(C.byref(m), st) == 0
    assert all(glue._untouched(*k) for k in keep if isinstance(k, tuple))
    return outs


# (B, H, E, T): a lane group with an idle lane at the smallest classes; B past one workgroup's rows, MoE <2, 4> against CGC
# <3, 4>; lgp = 64 with 33 columns, CGC <5, 4>; the column loop runs twice, E across a class bound; MoE's largest class
@pytest.mark.parametrize("B,H,E,T", [(33, 12, 2, 1), (70, 20, 3, 2), (33, 132, 4, 4), (70, 264, 5, 3), (33, 16, 8, 4)])
def test_an_moe_mix_is_a_cgc_mix_of_every_expert_bit_for_bit(dev, B, H, E, T):
    """tzr_moe_mix_* and tzr_cgc_mix_* with sel[g] = 0 .. E-1 for every gate are two instantiations of one kernel body
    (csrc/gate_mix.hip) with every sum in the same order: the same bits in out, probs, d_logits and d_expert"""
    import dense_glue_ref as ref

    xs, ls, gos = ref.draw_moe(B, H, E, T, seed=B * 151 + H * 11 + E * 5 + T)
    moe = run_abi(dev, xs, ls, gos, None)
    cgc = run_abi(dev, xs, ls, gos, [list(range(E))] * T)
    for kind in ("out", "probs", "d_logits", "d_expert"):
        assert len(moe[kind]) == len(cgc[kind]) == (E if kind == "d_expert" else T)
        for i, (a, b) in enumerate(zip(moe[kind], cgc[kind])):
            assert bool(torch.isfinite(a).all()), f"{kind}[{i}] of tzr_moe_mix is not finite"
            assert torch.equal(a, b), f"{kind}[{i}]: max abs difference {float((a - b).abs().max()):.3e}"
