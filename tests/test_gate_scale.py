"""gate_ops.gate_scale (tzr_gate_scale_fwd / _bwd, csrc/gate_scale.hip): out_n = act(z_n + bz_n) * gamma * sigmoid(g_n + bg_n) for
every slot of one PPNet level (or EPNet's one gate) in one launch per direction, against the literal expression evaluated in
float64 on the CPU.  Tolerances: out, dz, dg are elementwise kinds of tests/test_cgc_mix.py -- rtol 1e-5, atol 1e-6; the bias
gradients (sums over the batch) 4 x the distance of torch's own fp32 literal form to the float64 result on the same inputs,
floor 2^-20, relative to max(1, |want|)."""
import pytest
import torch

from cross_v2_ref import FLOOR, rel_err
from torcheasyrec_amd import _lib

GAMMA = 2.0
KINDS = ("out", "dz", "dg", "dbz", "dbg")


def literal(zs, bzs, gs, bgs, gouts, relu, dtype):
    """the literal expression with autograd on the CPU: dict kind -> list per slot; a slot without an output gradient gets
    zeros, a slot without bz no dbz entry"""
    leaf = lambda t: None if t is None else t.detach().cpu().to(dtype).clone().requires_grad_(True)  # noqa: E731
    zs, bzs, gs, bgs = ([leaf(t) for t in ts] for ts in (zs, bzs, gs, bgs))
    outs = []
    for z, bz, g, bg in zip(zs, bzs, gs, bgs):
        a = z if bz is None else z + bz
        outs.append((torch.relu(a) if relu else a) * (GAMMA * torch.sigmoid(g + bg)))
    pairs = [(o, go.detach().cpu().to(dtype)) for o, go in zip(outs, gouts) if go is not None]
    ins = [t for ts in (zs, bzs, gs, bgs) for t in ts if t is not None]
    grads = torch.autograd.grad([o for o, _ in pairs], ins, [go for _, go in pairs], allow_unused=True)
    by_id = {id(t): (torch.zeros_like(t) if gr is None else gr) for t, gr in zip(ins, grads)}
    return {"out": [o.detach() for o in outs], "dz": [by_id[id(t)] for t in zs], "dg": [by_id[id(t)] for t in gs],
            "dbz": [by_id[id(t)] for t in bzs if t is not None], "dbg": [by_id[id(t)] for t in bgs]}


def draw(B, H, N, relu, dev, seed, strided=False, with_bz=True):
    """z, dout ~ N(0,1); g ~ 3 N(0,1) with entries at +-40 and +-100; biases ~ 0.5 N(0,1); a few entries with z == -bz exactly;
    strided: column slices [:, 4 : 4 + H] of buffers 12 wider"""
    gen = torch.Generator().manual_seed(seed)

    def rows(scale=1.0):
        if strided:
            return (scale * torch.randn(B, H + 12, generator=gen)).to(dev)[:, 4:4 + H]
        return (scale * torch.randn(B, H, generator=gen)).to(dev)

    zs, gs, gouts = [rows() for _ in range(N)], [rows(3.0) for _ in range(N)], [rows() for _ in range(N)]
    bzs = [(0.5 * torch.randn(H, generator=gen)).to(dev) if with_bz else None for _ in range(N)]
    bgs = [torch.zeros(H).to(dev) for _ in range(N)]  # (zero, so that the planted +-40 / +-100 are what the sigmoid sees; drawn below for slot 0)
    bgs[0] = (0.5 * torch.randn(H, generator=gen)).to(dev) if N > 1 else bgs[0]
    sat = {}
    for n in range(N):
        spots = [(int(torch.randint(B, (1,), generator=gen)), int(torch.randint(H, (1,), generator=gen))) for _ in range(6)]
        for (b, h), v in zip(spots[:4], (40.0, -40.0, 100.0, -100.0)):
            gs[n][b, h] = v - float(bgs[n][h])
        sat[n] = (gs[n] + bgs[n]).abs() >= 99.0  # (the planted +-100, give or take the rounding of the bias add: far past saturation)
        if bzs[n] is not None:
            for b, h in spots[4:]:
                if (b, h) not in spots[:4]:
                    zs[n][b, h] = -bzs[n][h]
    leaf = lambda t: None if t is None else t.requires_grad_(True)  # noqa: E731
    return [leaf(t) for t in zs], [leaf(t) for t in bzs], [leaf(t) for t in gs], [leaf(t) for t in bgs], gouts, sat


def run(zs, bzs, gs, bgs, gouts, relu):
    from torcheasyrec_amd.gate_ops import gate_scale, gate_scale_ok

    assert gate_scale_ok(zs, gs, bzs, bgs)
    outs = gate_scale(zs, bzs, gs, bgs, GAMMA, relu)
    pairs = [(o, go) for o, go in zip(outs, gouts) if go is not None]
    ins = [t for ts in (zs, bzs, gs, bgs) for t in ts if t is not None]
    grads = torch.autograd.grad([o for o, _ in pairs], ins, [go for _, go in pairs], allow_unused=True)
    assert all(gr is not None for gr in grads)  # (one Function: every input gets a gradient, zeros where nothing flows)
    by_id = {id(t): gr for t, gr in zip(ins, grads)}
    return {"out": [o.detach() for o in outs], "dz": [by_id[id(t)] for t in zs], "dg": [by_id[id(t)] for t in gs],
            "dbz": [by_id[id(t)] for t in bzs if t is not None], "dbg": [by_id[id(t)] for t in bgs]}


# (B, H, N, relu): see the reasons beside each.  The kernel caps its grid at 512 row chunks; at H = 1024 a chunk is 4 rows (one row
# lane, four rows in flight), so 2052 rows are one workgroup's worth more than the cap: every chunk becomes 8 rows, the last one 4
SHAPES = [(1, 4, 1, False), (37, 8, 2, True), (70, 1024, 1, True),
          (513, 264, 8, True),   # 66 float4 columns: a partial last row-lane group; the slot maximum
          (4099, 64, 3, True),   # rows that are no multiple of the rows per sweep or per workgroup
          (2, 4096, 1, False),   # the widest row: four sweeps of 256 columns
          (2052, 1024, 1, True)]
CASES = [(*s, False) for s in SHAPES] + [(*s, True) for s in sorted(SHAPES, key=lambda s: s[0] * s[1] * s[2])[:4]]


@pytest.mark.parametrize("B,H,N,relu,strided", CASES)
def test_gate_scale_matches_the_literal_form(dev, B, H, N, relu, strided):
    with_bz = relu or H == 4096  # (EPNet's slot has no bias on z; the identity kernel takes one all the same)
    zs, bzs, gs, bgs, gouts, sat = draw(B, H, N, relu, dev, seed=B + H + N, strided=strided, with_bz=with_bz)
    if N > 1:
        gouts[1] = None  # one slot whose output gets no gradient
    got = run(zs, bzs, gs, bgs, gouts, relu)
    want = literal(zs, bzs, gs, bgs, gouts, relu, torch.float64)
    lit32 = literal(zs, bzs, gs, bgs, gouts, relu, torch.float32)
    what = f"B{B} H{H} N{N} relu={relu} strided={strided} on {dev.type}"
    for kind in KINDS:
        assert all(bool(torch.isfinite(t).all()) for t in got[kind]), f"{what} {kind}: not finite"
    for kind in ("out", "dz", "dg"):
        for i, (a, e) in enumerate(zip(got[kind], want[kind])):
            print(f"{what} {kind}[{i}]: max abs err {float((a.cpu().double() - e).abs().max()):.3e} (max |want| {float(e.abs().max()):.3e})")
            torch.testing.assert_close(a.cpu().double(), e, rtol=1e-5, atol=1e-6, msg=lambda m, k=kind, i=i: f"{what} {k}[{i}]: {m}")
    bad = []
    for kind in ("dbz", "dbg"):
        gap, err = rel_err(lit32[kind], want[kind]), rel_err(got[kind], want[kind])
        bound = max(4.0 * gap, FLOOR)
        print(f"{what} {kind}: err {err:.3e} torch fp32 literal gap {gap:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((kind, err, bound))
    assert not bad, f"{what}: {bad}"
    # saturation: dg is exactly 0 where g + bg = +-100; the ReLU's edge: dz is 0 where z == -bz
    for n, mask in sat.items():
        assert int(mask.sum()) >= 1 and float(got["dg"][n][mask].abs().max()) == 0.0, (what, n)
    if relu:
        for n in range(N):
            edge = (zs[n].detach() + bzs[n].detach()) == 0
            assert float(got["dz"][n][edge].abs().sum()) == 0.0 and float(got["out"][n][edge].abs().sum()) == 0.0
            assert int(edge.sum()) >= 1 or B * H < 8
    if N > 1:  # the slot without an output gradient: exact zeros everywhere
        assert float(got["dz"][1].abs().max()) == 0.0 and float(got["dg"][1].abs().max()) == 0.0
        assert float(got["dbg"][1].abs().max()) == 0.0 and float(got["dbz"][1].abs().max()) == 0.0
    again = run(zs, bzs, gs, bgs, gouts, relu)
    for kind in KINDS:
        assert all(torch.equal(a, b) for a, b in zip(got[kind], again[kind])), f"{what} {kind}: two runs differ"


def test_gate_scale_ok_refuses_what_the_kernel_does_not_take(dev):
    from torcheasyrec_amd.gate_ops import gate_scale_ok

    def case(B=6, H=8, N=2, dtype=torch.float32):
        new = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        return [new(B, H) for _ in range(N)], [new(B, H) for _ in range(N)], [new(H) for _ in range(N)], [new(H) for _ in range(N)]

    assert gate_scale_ok(*case()) and gate_scale_ok(*case(N=8)) and gate_scale_ok(*case(H=4096, N=1))
    assert not gate_scale_ok(*case(H=6)) and not gate_scale_ok(*case(H=4100)) and not gate_scale_ok(*case(N=9))
    assert not gate_scale_ok(*case(dtype=torch.float16)) and not gate_scale_ok(*case(B=0))
    zs, gs, bzs, bgs = case()
    odd = torch.zeros(6, 11, dtype=torch.float32, device=dev)[:, :8]  # an odd row stride
    assert not gate_scale_ok([zs[0], odd], gs, bzs, bgs) and not gate_scale_ok(zs, [odd, gs[1]], bzs, bgs)
    wide = torch.zeros(6, 20, dtype=torch.float32, device=dev)
    assert gate_scale_ok([zs[0], wide[:, 4:12]], gs, bzs, bgs) and not gate_scale_ok([zs[0], wide[:, 2:10]], gs, bzs, bgs)  # (misaligned rows)
    assert gate_scale_ok(zs, gs, [None, None], bgs) and not gate_scale_ok(zs, gs, bzs, [None, bgs[1]])
    assert _lib.GATE_SCALE_MAX_SLOTS == 8
