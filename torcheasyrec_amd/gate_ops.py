"""The gate steps of the multi-task models, one launch per direction for a whole level: the gate mix of MMoE and of PLE's CGC levels
(`moe_mix`, `cgc_mix`: csrc/gate_mix.hip), PEPNet's gate-and-scale (`gate_scale`: csrc/gate_scale.hip), DBMTL's relation-tower chain
(`relation_chain`: csrc/relation_chain.hip).  The caller asks an op's `*_ok` predicate first and runs the literal form where it refuses."""
from __future__ import annotations

import torch

from . import _lib


class _GateMixFn(torch.autograd.Function):
    """out_g = softmax(logits_g) . experts[sels[g]] for every gate of a layer in one launch per direction (csrc/gate_mix.hip);
    inputs: the member lists, the number of gates G, G gate-logit tensors [B, n_g], then E expert outputs [B, H].  `sels` None:
    every gate over every expert in logit-column order, MMoE's mixing step (tzr_moe_mix_fwd / _bwd); otherwise the gates of one
    CGC level of PLE (tzr_cgc_mix_fwd / _bwd).  Capturable: nothing reads the device, every buffer is torch's."""

    @staticmethod
    def _begin(sels, G, experts):
        """(the ABI's struct with sizes, experts and member lists filled, the stem of its entry points, the gates' widths)"""
        if sels is None:
            m, stem, widths = _lib.TzrMoeMix(), "tzr_moe_mix", [len(experts)] * G
            m.n_tasks = G
        else:
            m, stem, widths = _lib.TzrCgcMix(), "tzr_cgc_mix", [len(sel) for sel in sels]
            m.n_gates = G
            for g, sel in enumerate(sels):
                m.n_sel[g] = len(sel)
                for j, e in enumerate(sel):
                    m.sel[g][j] = e
        m.B, m.H, m.n_experts = *experts[0].shape, len(experts)
        for e, x in enumerate(experts):
            m.expert[e], m.expert_stride[e] = _lib.ptr(x), x.stride(0)
        return m, stem, widths

    @staticmethod
    def forward(ctx, sels, G, *tensors):
        logits = [t.contiguous() for t in tensors[:G]]
        experts = [_lib.rows16(t) for t in tensors[G:]]
        B, H = experts[0].shape
        dev = experts[0].device
        m, stem, widths = _GateMixFn._begin(sels, G, experts)
        outs = [torch.empty(B, H, dtype=torch.float32, device=dev) for _ in range(G)]
        probs = [torch.empty(B, n, dtype=torch.float32, device=dev) for n in widths]
        for g in range(G):
            m.logits[g], m.logits_stride[g] = _lib.ptr(logits[g]), logits[g].stride(0)
            m.probs[g] = _lib.ptr(probs[g])
            m.out[g], m.out_stride[g] = _lib.ptr(outs[g]), outs[g].stride(0)
        _lib.launch(stem + "_fwd", m, dev)
        ctx.save_for_backward(*probs, *experts)
        ctx.sels, ctx.n_gates = sels, G
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        G = ctx.n_gates
        probs, experts = ctx.saved_tensors[:G], ctx.saved_tensors[G:]
        B, H = experts[0].shape
        dev = experts[0].device
        gs = [torch.zeros(B, H, dtype=torch.float32, device=dev) if g is None else _lib.rows16(g.float()) for g in gouts]
        m, stem, widths = _GateMixFn._begin(ctx.sels, G, experts)
        dx = [torch.empty(B, H, dtype=torch.float32, device=dev) for _ in experts]
        dl = [torch.empty(B, n, dtype=torch.float32, device=dev) for n in widths]
        for e in range(len(experts)):
            m.d_expert[e], m.d_expert_stride[e] = _lib.ptr(dx[e]), dx[e].stride(0)
        for g in range(G):
            m.probs[g] = _lib.ptr(probs[g])
            m.grad_out[g], m.grad_out_stride[g] = _lib.ptr(gs[g]), gs[g].stride(0)
            m.d_logits[g], m.d_logits_stride[g] = _lib.ptr(dl[g]), dl[g].stride(0)
        _lib.launch(stem + "_bwd", m, dev)
        return (None, None, *dl, *dx)


def _gate_mix_shapes_ok(logits, experts, widths, max_experts, max_gates) -> bool:
    """the shape rules tzr_moe_mix_* and tzr_cgc_mix_* share: fp32 experts [B, H] (B > 0, H % 4 == 0, <= 4096, at most
    `max_experts`), at most `max_gates` gates, gate g with fp32 logits [B, widths[g]]"""
    if not (0 < len(experts) <= max_experts and 0 < len(logits) <= max_gates and len(widths) == len(logits)):
        return False
    x = experts[0]
    return bool(x.dim() == 2 and x.shape[0] > 0 and x.shape[1] % 4 == 0 and 0 < x.shape[1] <= 4096
                and all(t.dtype == torch.float32 and t.shape == x.shape for t in experts)
                and all(t.dtype == torch.float32 and n > 0 and t.shape == (x.shape[0], n) for t, n in zip(logits, widths)))


def moe_mix_ok(logits, experts) -> bool:
    """what tzr_moe_mix_* takes (the device and the backend are the caller's to look at)"""
    return _gate_mix_shapes_ok(logits, experts, [len(experts)] * len(logits), _lib.MOE_MAX_EXPERTS, _lib.MOE_MAX_TASKS)


def moe_mix(logits, experts):
    """[softmax(logits_t) . experts for t] -- the mixing step of MMoE (tzrec/modules/mmoe.py:63-76) -- one launch for all tasks."""
    return list(_GateMixFn.apply(None, len(logits), *logits, *experts))


def cgc_mix_ok(logits, experts, sels) -> bool:
    """what tzr_cgc_mix_* takes: the shared shape rules at its limits (at most 16 experts, 5 gates), gate g over distinct
    experts sels[g], everything on the device of the loaded library"""
    if not _gate_mix_shapes_ok(logits, experts, [len(sel) for sel in sels], _lib.CGC_MAX_EXPERTS, _lib.CGC_MAX_GATES):
        return False
    dev = experts[0].device
    if not all(t.device == dev for t in (*experts, *logits)) or not _lib.takes(dev):
        return False
    return all(len(set(sel)) == len(sel) and all(0 <= int(e) < len(experts) for e in sel) for sel in sels)


def cgc_mix(logits, experts, sels):
    """[softmax(logits_g) . [experts[e] for e in sels[g]] for g] -- the gate-and-mix step of one CGC level of PLE
    (tzrec/modules/extraction_net.py:98-139) -- one launch for all gates; an expert of several gates is read once."""
    sels = tuple(tuple(int(e) for e in sel) for sel in sels)
    return list(_GateMixFn.apply(sels, len(sels), *logits, *experts))


class _GateScaleFn(torch.autograd.Function):
    """out_n = act(z_n + bz_n) * gamma * sigmoid(g_n + bg_n) for every slot (task of one PPNet level, or EPNet's one gate) in one
    launch per direction plus the bias gradients' finishing launch (tzr_gate_scale_fwd / _bwd, csrc/gate_scale.hip); inputs: N
    tensors z [B, H], N biases bz ([H] or None), N tensors g [B, H], N biases bg [H].  Saved for the backward: the inputs, nothing
    the forward computed.  Capturable: nothing reads the device, every buffer is torch's."""

    @staticmethod
    def _fill(m, B, H, gamma, relu, zs, bzs, gs, bgs):
        m.B, m.H, m.n_slots, m.relu, m.gamma = B, H, len(zs), 1 if relu else 0, gamma
        for n, (z, bz, g, bg) in enumerate(zip(zs, bzs, gs, bgs)):
            m.z[n], m.z_stride[n] = _lib.ptr(z), z.stride(0)
            m.g[n], m.g_stride[n] = _lib.ptr(g), g.stride(0)
            m.bz[n], m.bg[n] = _lib.opt_ptr(bz), _lib.ptr(bg)

    @staticmethod
    def forward(ctx, gamma, relu, N, *tensors):
        zs, bzs, gs, bgs = tensors[:N], tensors[N:2 * N], tensors[2 * N:3 * N], tensors[3 * N:]
        B, H = zs[0].shape
        dev = zs[0].device
        m = _lib.TzrGateScale()
        _GateScaleFn._fill(m, B, H, gamma, relu, zs, bzs, gs, bgs)
        outs = [torch.empty(B, H, dtype=torch.float32, device=dev) for _ in range(N)]
        for n in range(N):
            m.out[n], m.out_stride[n] = _lib.ptr(outs[n]), outs[n].stride(0)
        _lib.launch("tzr_gate_scale_fwd", m, dev)
        ctx.save_for_backward(*zs, *bzs, *gs, *bgs)
        ctx.gamma, ctx.relu, ctx.N = gamma, relu, N
        ctx.set_materialize_grads(False)  # (a slot without an output gradient: a null pointer, not a [B, H] fill)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        N = ctx.N
        t = ctx.saved_tensors
        zs, bzs, gs, bgs = t[:N], t[N:2 * N], t[2 * N:3 * N], t[3 * N:]
        B, H = zs[0].shape
        dev = zs[0].device
        gos = [None if g is None else _lib.rows16(g.float()) for g in gouts]
        m = _lib.TzrGateScale()
        _GateScaleFn._fill(m, B, H, ctx.gamma, ctx.relu, zs, bzs, gs, bgs)
        dz = [torch.empty(B, H, dtype=torch.float32, device=dev) for _ in range(N)]
        dg = [torch.empty(B, H, dtype=torch.float32, device=dev) for _ in range(N)]
        db = torch.empty(N, 2, H, dtype=torch.float32, device=dev)
        ws = _lib.workspace(_lib.lib().tzr_gate_scale_bwd_workspace(B, H, N), dev)  # (sized by the shape, not by the struct)
        for n in range(N):
            if gos[n] is not None:
                m.grad_out[n], m.grad_out_stride[n] = _lib.ptr(gos[n]), gos[n].stride(0)
            m.dz[n], m.dz_stride[n] = _lib.ptr(dz[n]), dz[n].stride(0)
            m.dg[n], m.dg_stride[n] = _lib.ptr(dg[n]), dg[n].stride(0)
        m.d_bias, m.ws, m.ws_bytes = _lib.ptr(db), _lib.ptr(ws), ws.numel()
        _lib.launch("tzr_gate_scale_bwd", m, dev)
        dbz = [None if bzs[n] is None else db[n, 0] for n in range(N)]
        return (None, None, None, *dz, *dbz, *dg, *[db[n, 1] for n in range(N)])


def gate_scale_ok(zs, gs, bzs=None, bgs=None) -> bool:
    """what tzr_gate_scale_* takes: 1 to 8 slots of fp32 z and g [B, H] (B > 0, H % 4 == 0, <= 4096) with unit column stride, row
    strides that are multiples of 4 floats and 16-byte aligned rows -- column slices of wider buffers are fine --, contiguous
    aligned fp32 biases [H] (a bz may be None), everything on the device of the loaded library"""
    if not (0 < len(zs) <= _lib.GATE_SCALE_MAX_SLOTS and len(gs) == len(zs)):
        return False
    x = zs[0]
    if not (x.dim() == 2 and x.shape[0] > 0 and x.shape[1] % 4 == 0 and 0 < x.shape[1] <= 4096):
        return False
    (B, H), dev = x.shape, x.device
    if not _lib.takes(dev):
        return False
    for t in (*zs, *gs):
        if not (_lib.rows_ok(t, H) and t.shape[0] == B and t.device == dev):
            return False
    for bs, nullable in ((bzs, True), (bgs, False)):
        if bs is not None and (len(bs) != len(zs)
                               or not all(nullable if b is None else _lib.packed_ok(b, (H,), dev, aligned=True) for b in bs)):
            return False
    return True


def gate_scale(zs, bzs, gs, bgs, gamma: float, relu: bool):
    """[act(z_n + bz_n) * gamma * sigmoid(g_n + bg_n) for n] -- what follows the three GEMMs of every task of one PPNet level, or
    of EPNet (tzrec/modules/personalized_net.py) -- one launch for all slots; `zs` / `gs` are the GEMM outputs WITHOUT bias.  The
    caller checks `gate_scale_ok(zs, gs, bzs, bgs)` first."""
    N = len(zs)
    return list(_GateScaleFn.apply(float(gamma), bool(relu), N, *zs, *bzs, *gs, *bgs))


class _RelationChainFn(torch.autograd.Function):
    """Every Bayesian relation tower of a DBMTL model in one launch forward and two backward (tzr_relation_chain_fwd / _bwd,
    csrc/relation_chain.hip).  `deps[t]`: the earlier towers tower t reads; `n_layers[t]`: its layers (0: r_t = x_t).  Inputs: T
    tensors x_t, then per tower with layers its (weight, bias) pairs in order.  Outputs: every layer's post-ReLU output, tower-
    major; the last of a tower is r_t, the others carry no gradient.  Saved for the backward: the inputs and those outputs.
    Capturable: the struct is read when the launch is recorded, every buffer is torch's."""

    @staticmethod
    def _fill(m, xs, deps, n_layers, params, hs):
        B = xs[0].shape[0]
        m.B, m.n_towers = B, len(xs)
        k = 0
        for t, x in enumerate(xs):
            m.x[t], m.x_stride[t], m.x_width[t] = _lib.ptr(x), x.stride(0), x.shape[1]
            m.n_layers[t], m.n_deps[t] = n_layers[t], len(deps[t])
            for j, d in enumerate(deps[t]):
                m.deps[t][j] = d
            for l in range(n_layers[t]):
                w, b = params[2 * k], params[2 * k + 1]
                m.width[t][l] = w.shape[0]
                m.w[t][l], m.b[t][l], m.h[t][l] = _lib.ptr(w), _lib.ptr(b), _lib.ptr(hs[k])
                k += 1

    @staticmethod
    def forward(ctx, deps, n_layers, *tensors):
        T = len(n_layers)
        xs, params = tensors[:T], [p.contiguous() for p in tensors[T:]]
        B, dev = xs[0].shape[0], xs[0].device
        hs = [torch.empty(B, params[2 * k].shape[0], dtype=torch.float32, device=dev) for k in range(len(params) // 2)]
        m = _lib.TzrRelationChain()
        _RelationChainFn._fill(m, xs, deps, n_layers, params, hs)
        _lib.launch("tzr_relation_chain_fwd", m, dev)
        ctx.save_for_backward(*xs, *params, *hs)
        ctx.deps, ctx.n_layers = deps, n_layers
        last = {sum(n_layers[:t + 1]) - 1 for t in range(T) if n_layers[t]}
        hidden = [h for k, h in enumerate(hs) if k not in last]
        if hidden:
            ctx.mark_non_differentiable(*hidden)
        ctx.set_materialize_grads(False)  # (a tower without an outside gradient: a null pointer, not a [B, N] fill)
        return tuple(hs)

    @staticmethod
    def backward(ctx, *gouts):
        deps, n_layers = ctx.deps, ctx.n_layers
        T, n = len(n_layers), sum(n_layers)
        saved = ctx.saved_tensors
        xs, params, hs = saved[:T], saved[T:T + 2 * n], saved[T + 2 * n:]
        B, dev = xs[0].shape[0], xs[0].device
        m = _lib.TzrRelationChain()
        _RelationChainFn._fill(m, xs, deps, n_layers, params, hs)
        dxs = [torch.empty(B, x.shape[1], dtype=torch.float32, device=dev) for x in xs]
        dps = [torch.empty_like(p) for p in params]
        keep, k = [], 0
        for t in range(T):
            m.dx[t], m.dx_stride[t] = _lib.ptr(dxs[t]), dxs[t].stride(0)
            for l in range(n_layers[t]):
                m.dw[t][l], m.db[t][l] = _lib.ptr(dps[2 * k]), _lib.ptr(dps[2 * k + 1])
                k += 1
            if n_layers[t] and gouts[k - 1] is not None:
                g = _lib.rows16(gouts[k - 1].float())
                keep.append(g)
                m.grad_r[t], m.grad_r_stride[t] = _lib.ptr(g), g.stride(0)
        _lib.launch_ws("tzr_relation_chain_bwd", m, dev, "tzr_relation_chain_bwd")
        return (None, None, *dxs, *dps)


def relation_chain_ok(xs, deps, layers) -> bool:
    """what tzr_relation_chain_* takes: 1 to 8 towers; fp32 x_t [B, Hx] (B > 0, Hx % 4 == 0, <= 1024) with unit column stride, row
    strides that are multiples of 4 floats and 16-byte aligned rows -- column slices of wider buffers are fine --; `deps[t]`
    distinct earlier towers; `layers[t]` 0 to 4 (weight [N, K], bias [N]) pairs, fp32, N % 4 == 0, <= 128, K the width of the
    layer's input (layer 0: Hx plus the widths of the deps' outputs); everything on the device of the loaded library"""
    T = len(xs)
    if not (0 < T <= _lib.RELATION_CHAIN_MAX_TOWERS and len(deps) == T and len(layers) == T):
        return False
    x0 = xs[0]
    if not (x0.dim() == 2 and x0.shape[0] > 0) or not _lib.takes(x0):
        return False
    B, dev = x0.shape[0], x0.device
    widths = []
    for t in range(T):
        x, lay = xs[t], layers[t]
        if not (_lib.rows_ok(x) and x.device == dev and x.shape[0] == B and x.shape[1] % 4 == 0
                and 0 < x.shape[1] <= _lib.RELATION_CHAIN_MAX_X):
            return False
        if len(lay) > _lib.RELATION_CHAIN_MAX_LAYERS:
            return False
        ds = [int(d) for d in deps[t]]
        if len(set(ds)) != len(ds) or not all(0 <= d < t for d in ds):
            return False
        K = x.shape[1] + sum(widths[d] for d in ds)
        for w, b in lay:
            N = w.shape[0]
            if not (N % 4 == 0 and 0 < N <= _lib.RELATION_CHAIN_MAX_WIDTH and _lib.packed_ok(w, (N, K), dev, aligned=True)
                    and b is not None and _lib.packed_ok(b, (N,), dev, aligned=True)):
                return False
            K = N
        widths.append(K if lay else x.shape[1])
    return True


def relation_chain(xs, deps, layers, hidden: bool = False):
    """[r_t for t]: r_t = xs[t] itself for a tower without layers, else the ReLU MLP `layers[t]` over the virtual concatenation
    [xs[t] | r_d for d in deps[t]] -- the relation towers of DBMTL (tzrec/models/dbmtl.py:155-167) -- one launch for the whole
    chain, no concat tensor.  `hidden`: also every layer's output, [[h_{t,l} for l] for t].  The caller checks
    `relation_chain_ok(xs, deps, layers)` first."""
    n_layers = tuple(len(lay) for lay in layers)
    deps = tuple(tuple(int(d) for d in ds) if n else () for ds, n in zip(deps, n_layers))
    flat = [p for lay in layers for wb in lay for p in wb]
    hs = _RelationChainFn.apply(deps, n_layers, *xs, *flat) if sum(n_layers) else ()
    out, per, k = [], [], 0
    for t, n in enumerate(n_layers):
        per.append(list(hs[k:k + n]))
        k += n
        out.append(hs[k - 1] if n else xs[t])
    return (out, per) if hidden else out
