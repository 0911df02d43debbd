"""Restatement of DBMTL's relation towers for the tests (tzrec/models/dbmtl.py:155-167), in plain torch on the CPU in the dtype
asked for: per tower with layers the literal `torch.cat([x_t] + [r_d for d in deps_t], dim=1)` through Linear + ReLU layers, a
tower without layers passing its input on; gradients by autograd.  In float64 it is the truth the kernel is held to; in float32
it is the yardstick (`gap`): the literal form's own distance to float64 on the same inputs.  Nothing here touches the package
under test.

The ReLU masks are internal to the chain, so `settle` redraws the rows that leave ANY float64 pre-activation within MARGIN of
zero, where fp32 could take the other side -- a condition on the inputs, checked with the reference alone; no element is ever
left out of a comparison."""
import torch
import torch.nn.functional as F

from mlp_ref import check, rel_err  # noqa: F401  (the project's one bound: max(4 x gap, 2^-20) per kind, NaN-aware)

KINDS = ("h", "dx", "dW", "db")
MARGIN = 2.0 ** -12
MAX_PASSES = 200


def unique(ts):
    """the distinct tensors of a list, in order of first appearance (two towers may share one x)"""
    seen, out = set(), []
    for t in ts:
        if id(t) not in seen:
            seen.add(id(t))
            out.append(t)
    return out


def forward(xs, deps, layers):
    """-> (r per tower, h per tower and layer, pre-activations per tower and layer), in the dtype of the arguments"""
    rs, hs, pres = [], [], []
    for x, ds, lay in zip(xs, deps, layers):
        h, ht, pt = x, [], []
        if lay:
            h = torch.cat([x] + [rs[d] for d in ds], dim=1)
        for w, b in lay:
            pre = F.linear(h, w, b)
            h = torch.relu(pre)
            pt.append(pre)
            ht.append(h)
        rs.append(h)
        hs.append(ht)
        pres.append(pt)
    return rs, hs, pres


def literal(xs, deps, layers, gouts, dtype=torch.float64):
    """xs: T tensors [B, Hx] (the same object twice: one shared input); layers[t]: (W, b) pairs; gouts[t]: dL/dr_t or None ->
    kind -> list: h tower-major, dx per DISTINCT x, dW / db tower-major"""
    leaves = {id(t): t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in unique(xs)}
    lx = [leaves[id(t)] for t in xs]
    ll = [[(w.detach().cpu().to(dtype).clone().requires_grad_(True), b.detach().cpu().to(dtype).clone().requires_grad_(True)) for w, b in lay]
          for lay in layers]
    rs, hs, _ = forward(lx, deps, ll)
    pairs = [(r, g.detach().cpu().to(dtype)) for r, g in zip(rs, gouts) if g is not None]
    ins = unique(lx) + [p for lay in ll for wb in lay for p in wb]
    grads = torch.autograd.grad([r for r, _ in pairs], ins, [g for _, g in pairs], allow_unused=True) if pairs else [None] * len(ins)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(ins, grads)]
    n = len(unique(lx))
    return {"h": [h.detach() for ht in hs for h in ht], "dx": grads[:n], "dW": grads[n::2], "db": grads[n + 1::2]}


def gaps(xs, deps, layers, gouts, want64):
    r32 = literal(xs, deps, layers, gouts, torch.float32)
    return {k: rel_err(r32[k], want64[k]) for k in KINDS}


def margin_rows(xs, deps, layers):
    """bool [B]: the rows with a float64 pre-activation within MARGIN of zero"""
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    _, _, pres = forward([d(x) for x in xs], deps, [[(d(w), d(b)) for w, b in lay] for lay in layers])
    bad = torch.zeros(xs[0].shape[0], dtype=torch.bool)
    for pt in pres:
        for pre in pt:
            bad |= (pre.abs() < MARGIN).any(dim=1)
    return bad


def settle(xs, deps, layers, g, scale=1.0):
    """redraws (scale N(0, 1), generator `g`), in place, the rows of every x that break the margin condition, until none does"""
    for n in range(MAX_PASSES + 1):
        bad = margin_rows(xs, deps, layers)
        if not bool(bad.any()):
            return xs
        assert n < MAX_PASSES, f"{int(bad.sum())} rows still break the margin condition after {MAX_PASSES} passes"
        for x in unique(xs):
            x[bad] = scale * torch.randn(int(bad.sum()), x.shape[1], generator=g)
    return xs


def draw(B, hx, deps, widths, seed, shared=None):
    """x ~ N(0, 1), settled; weights and biases uniform within nn.Linear's default bounds; g_t ~ N(0, 1) / sqrt(B) for every
    tower.  `shared`: {t: s} tower t reads the x object of tower s -> xs, layers, gouts (CPU tensors).

    Why 1 / sqrt(B): dW and db are sums over the batch, and the error measure divides by max(1, |fp64|).  With g ~ N(0, 1) the
    partial sums of B = 8209 terms reach about sqrt(B) = 90 whatever the order, every addition up there rounds by up to
    ulp(64) / 2 = 3.8e-6, and an entry that happens to END near zero is then held to that error over 1 -- more than the bound for
    ANY fp32 summation, torch's literal form included (its own entries miss by up to 3e-5 absolute at that scale).  Scaled so
    that the sums are of order 1 -- what a loss that is a mean over the batch sends, up to the remaining sqrt(B) -- every entry
    sits where relative and absolute error coincide, and the bound asks for six digits of each of them."""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for t, w in enumerate(hx):
        xs.append(xs[shared[t]] if shared and t in shared else torch.randn(B, w, generator=g))
    layers, rw = [], []
    for t, ws in enumerate(widths):
        K = hx[t] + sum(rw[d] for d in deps[t])
        lay = []
        for N in ws:
            bound = K ** -0.5
            lay.append(((torch.rand(N, K, generator=g) * 2 - 1) * bound, (torch.rand(N, generator=g) * 2 - 1) * bound))
            K = N
        layers.append(lay)
        rw.append(K if ws else hx[t])
    settle(xs, deps, layers, g)
    gouts = [torch.randn(B, w, generator=g) / B ** 0.5 for w in rw]
    return xs, layers, gouts
