"""Generate tests/golden/reference_loss_vectors.npz by RUNNING the reference's own loss modules.

Run in the authoring container only (needs /root/reference; the GPU box has none):

    python tests/golden/make_reference_loss_vectors.py

tzrec/loss/jrc_loss.py (JRCLoss) and tzrec/loss/focal_loss.py (BinaryFocalLoss) are plain torch; they are imported from where
they lie through the import shim of make_reference_module_vectors.py and run on CPU twice per case: in fp32, and with the
logits in double (JRCLoss(reduction="none") cannot: the fp64 side of its weighted form is tests/loss_ref.py's closed form).  Stored per case: the inputs, the fp32 and fp64 loss of `reduction="mean"`, both gradients, and the same
for `reduction="none"` combined with a weight vector as RankModel._loss_impl does (mean(l * div_no_nan(w, mean(w)))).  The
8-row / 2-session case is the one of the reference's jrc_loss_test.py, read from that file when this script runs (expected
value 0.7199).

`ref_gap/<kind>/{loss,grad}`: the largest |fp32 - fp64| / max(1, |fp64|) of the losses, and the largest |fp32 - fp64| of
B * gradient, over the kind's cases -- for jrc_loss and binary_focal_loss from the reference's modules, for
binary_cross_entropy, softmax_cross_entropy and l2_loss (compared with tests/loss_ref.py only) from torch.nn.functional in
fp32 against fp64 on the inputs tests/test_losses.py draws (tests/loss_ref.py's generators).  The tests' bounds are 4 x these.
"""
import ast
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import loss_ref as ref  # noqa: E402
from make_reference_module_vectors import REF, install_reference_imports  # noqa: E402


def _np(t):
    return t.detach().cpu().numpy().copy()


def _run(module, args, logits, dtype, weight=None):
    """(loss, gradient) of the module on logits cast to `dtype`; with `weight`: reduction="none" rows combined as _loss_impl does"""
    x = logits.detach().to(dtype).requires_grad_(True)
    out = module(x, *[a.to(dtype) if a.is_floating_point() else a for a in args])  # (float labels follow the logits' precision)
    if weight is not None:
        w = weight.to(dtype)
        m = torch.mean(w)
        w = torch.where(m == 0, torch.zeros_like(w), w / m)  # div_no_nan
        out = torch.mean(out * w)
    (g,) = torch.autograd.grad(out, x)
    return out.detach(), g.detach()


class _Gap:
    def __init__(self):
        self.loss, self.grad = 0.0, 0.0

    def add(self, l32, l64, g32, g64):
        B = g64.shape[0]
        self.loss = max(self.loss, float((l32.double() - l64).abs() / max(1.0, float(l64.abs()))))
        self.grad = max(self.grad, float((g32.double() - g64).abs().max()) * B)


def _literal_case():
    """the tensors of JRCLossTest.test_jrc_loss, read from the reference's test file"""
    tree = ast.parse(open(os.path.join(REF, "loss", "jrc_loss_test.py")).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "test_jrc_loss")
    lists = [ast.literal_eval(c.args[0]) for c in ast.walk(fn) if isinstance(c, ast.Call) and getattr(c.func, "attr", "") == "tensor"]
    expected = next(ast.literal_eval(c.args[0]) for c in ast.walk(fn) if isinstance(c, ast.Call) and getattr(c.func, "attr", "") == "assertEqual")
    logits, labels, sids = lists
    return torch.tensor(logits, dtype=torch.float32), torch.tensor(labels), torch.tensor(sids, dtype=torch.int64), float(expected)


def main():
    install_reference_imports()
    m = types.ModuleType("tzrec.loss")
    m.__path__ = [REF + "/loss"]
    sys.modules["tzrec.loss"] = m
    JRCLoss = importlib.import_module("tzrec.loss.jrc_loss").JRCLoss
    BinaryFocalLoss = importlib.import_module("tzrec.loss.focal_loss").BinaryFocalLoss
    torch.set_num_threads(1)
    out, gaps = {}, {k: _Gap() for k in ref.ROWS}

    def store(tag, kind, make, args, logits, weight, keep=True, closed64=None):
        for form, w in (("mean", None), ("weighted", weight)):
            red = "mean" if w is None else "none"
            l32, g32 = _run(make(red), args, logits, torch.float32, w)
            if w is not None and closed64 is not None:
                # JRCLoss(reduction="none") builds its row tensor in float32 whatever the logits are and cannot take double
                # logits: the fp64 side of its weighted form is tests/loss_ref.py's closed form, which
                # tests/test_losses.py holds to the module's own fp64 mean form at 1e-12
                l64, g64 = closed64(w)
            else:
                l64, g64 = _run(make(red), args, logits, torch.float64, w)
            gaps[kind].add(l32, l64, g32, g64)
            for k, v in (("loss32", l32), ("loss64", l64), ("grad32", g32), ("grad64", g64)) if keep else ():
                out[f"{tag}/{form}/{k}"] = _np(v)

    # jrc_loss: (B, sessions, logit scale, alpha); every batch holds both classes (the mean form is NaN otherwise)
    jrc_cases = [(8, 1, 1.0, 0.5), (16, 3, 1.0, 0.5), (64, 5, 8.0, 0.2), (65, 65, 1.0, 0.5), (300, 17, 8.0, 0.5), (1024, 97, 1.0, 0.2)]
    names = []
    for B, S, scale, alpha in jrc_cases:
        x, y, sid = ref.jrc_inputs(B, S, scale)
        y[0], y[-1] = 1, 0
        w, _ = ref.weight_inputs(B)
        tag = f"jrc/B{B}_S{S}_x{int(scale)}_a{alpha}"
        names.append(tag)
        out[f"{tag}/logits"], out[f"{tag}/labels"], out[f"{tag}/session"], out[f"{tag}/weight"] = _np(x), _np(y), _np(sid), _np(w)
        out[f"{tag}/alpha"] = np.float64(alpha)
        store(tag, "jrc_loss", lambda red, a=alpha: JRCLoss(alpha=a, reduction=red), (y, sid), x, w,
              closed64=lambda ww, x=x, y=y, sid=sid, a=alpha: ref.loss_and_grad("jrc_loss", x, y, sid, alpha=a, weight=ww))
    x, y, sid, expected = _literal_case()
    tag = "jrc/literal"
    names.append(tag)
    out[f"{tag}/logits"], out[f"{tag}/labels"], out[f"{tag}/session"] = _np(x), _np(y), _np(sid)
    out[f"{tag}/weight"], out[f"{tag}/alpha"], out[f"{tag}/expected"] = _np(ref.weight_inputs(8)[0]), np.float64(0.5), np.float64(expected)
    store(tag, "jrc_loss", lambda red: JRCLoss(reduction=red), (y, sid), x, ref.weight_inputs(8)[0],
          closed64=lambda ww: ref.loss_and_grad("jrc_loss", x, y, sid, alpha=0.5, weight=ww))
    assert round(float(out[f"{tag}/mean/loss32"]), 4) == expected
    out["jrc/cases"] = np.array(names)

    # binary_focal_loss: the (B, scale, gamma, alpha) grid of the tests
    names = []
    for B in ref.POINTWISE_B:
        for scale in ref.SCALES:
            for gamma, alpha in ref.FOCAL_PARAMS:
                x, y, _ = ref.pointwise_inputs(B, scale)
                w, _ = ref.weight_inputs(B)
                tag = f"focal/B{B}_x{int(scale)}_g{gamma}_a{alpha}"
                keep = B <= 1025  # (the 4097-row cases count in ref_gap; their vectors would not fit a committed file)
                if keep:
                    names.append(tag)
                    out[f"{tag}/logits"], out[f"{tag}/labels"], out[f"{tag}/weight"] = _np(x), _np(y), _np(w)
                    out[f"{tag}/gamma"], out[f"{tag}/alpha"] = np.float64(gamma), np.float64(alpha)
                store(tag, "binary_focal_loss", lambda red, g=gamma, a=alpha: BinaryFocalLoss(gamma=g, alpha=a, reduction=red),
                      (y.float(),), x, w, keep)
    out["focal/cases"] = np.array(names)

    # the kinds compared with tests/loss_ref.py only: torch's own fp32 functional against fp64, on the tests' inputs
    def functional(kind, fn, x, args):
        w, _ = ref.weight_inputs(x.shape[0])
        for weight in (None, w):
            red = "mean" if weight is None else "none"
            mod = lambda t, *a: fn(t, *[v.to(t.dtype) if v.is_floating_point() else v for v in a], reduction=red)  # noqa: E731
            l32, g32 = _run(mod, args, x, torch.float32, weight)
            l64, g64 = _run(mod, args, x, torch.float64, weight)
            gaps[kind].add(l32, l64, g32, g64)

    for B in ref.POINTWISE_B:
        for scale in ref.SCALES:
            x, y, t = ref.pointwise_inputs(B, scale)
            for s in (0.0, 0.1):
                functional("binary_cross_entropy", F.binary_cross_entropy_with_logits, x, (y.float() * (1 - s) + 0.5 * s,))
            functional("l2_loss", F.mse_loss, x, (t,))
    for B in ref.SOFTMAX_B:
        for C in ref.SOFTMAX_C:
            x, y = ref.softmax_inputs(B, C)
            for eps in (0.0, 0.1):
                functional("softmax_cross_entropy", lambda t, yy, reduction, e=eps: F.cross_entropy(t, yy, reduction=reduction, label_smoothing=e), x, (y,))
    for kind, g in gaps.items():
        out[f"ref_gap/{kind}/loss"], out[f"ref_gap/{kind}/grad"] = np.float64(g.loss), np.float64(g.grad)
        print(f"ref_gap {kind}: loss {g.loss:.3e}  B*grad {g.grad:.3e}")
    path = os.path.join(HERE, "reference_loss_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
