"""What the dense-optimizer tests compare against: the same gradient sequence through torch.optim's single-tensor path in
float64 and in float32 on the CPU, and the bound the fused result has to keep.

The bound is derived, not chosen: the fused result's largest deviation from the float64 run may be at most 4x the float32 CPU
run's largest deviation from it (the margin is for fma contraction and sqrtf / division rounding, which differ between the CPU
and the device), plus a floor of one fp32 ulp of the parameter scale (a float32 run that happens to round like float64 would
otherwise leave no room at all)."""
import numpy as np
import torch

TORCH_CLASS = {"sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW,
               "adadelta": torch.optim.Adadelta, "rmsprop": torch.optim.RMSprop}


def torch_optimizer(kind, params, **opts):
    """torch.optim's single-tensor (foreach=False) implementation of `kind`"""
    return TORCH_CLASS[kind](params, foreach=False, **opts)


class Reference:
    """parameters stepped by torch.optim on the CPU in `dtype`, fed gradients tensor by tensor (None: no gradient this step)"""

    def __init__(self, kind, init, dtype, **opts):
        self.params = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in init]
        self.opt = torch_optimizer(kind, self.params, **opts)
        self.dtype = dtype

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else g.detach().cpu().to(self.dtype).clone()
        self.opt.step()

    def values(self):
        return [p.detach().double() for p in self.params]


def max_dev(values, exact):
    return max(float((v.detach().cpu().double() - e).abs().max()) for v, e in zip(values, exact))


def check_bound(fused, f32, f64, what=""):
    """prints both deviations, then asserts the bound of this module's docstring; returns (fused deviation, float32 deviation)"""
    d_fused, d_f32 = max_dev(fused, f64), max_dev(f32, f64)
    scale = max(float(e.abs().max()) for e in f64)
    floor = float(np.spacing(np.float32(scale)))
    print(f"[dense-optim] {what}: fused max|dev| vs float64 = {d_fused:.3e}, float32 CPU max|dev| = {d_f32:.3e}, "
          f"bound = 4 x {d_f32:.3e} + ulp({scale:.3g}) = {4 * d_f32 + floor:.3e}")
    assert d_fused <= 4 * d_f32 + floor, (what, d_fused, d_f32, floor)
    return d_fused, d_f32
