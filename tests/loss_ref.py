"""Pure-torch float64 restatement of the configured losses: what tests/test_losses.py and tests/test_loss_config.py compare
`torcheasyrec_amd.losses` against, and the inputs both they and tests/golden/make_reference_loss_vectors.py draw.

* binary_cross_entropy (label_smoothing s; the smoothed label is float32, as the reference's is), softmax_cross_entropy (label_smoothing), l2_loss: torch.nn.functional in double.
* binary_focal_loss: f = alpha y (1-p)^gamma + (1-alpha)(1-y) p^gamma with p = sigmoid(x), DETACHED, times the BCE.
* jrc_loss: per session s, A_s = logsumexp of l1 over its negatives, B_s = logsumexp of l0 over its positives (-inf when
  empty); ge_i = softplus(A_s - l1_i) for a positive row, softplus(B_s - l0_i) for a negative; row = alpha CE + (1 - alpha) ge.
* weights: w_i = weight_i * (space_label_i > 0 ? in_w : out_w); loss = task_weight * sum(w l) / sum(w), 0 when sum(w) == 0
  (the reference's mean(l * div_no_nan(w, mean(w))) * weight).
Gradients are autograd's of these expressions.
"""
import torch
import torch.nn.functional as F

POINTWISE_B = (1, 63, 1024, 1025, 4097)
SCALES = (1.0, 30.0)
FOCAL_PARAMS = ((2.0, 0.5), (0.0, 0.25), (1.5, 0.75))
SOFTMAX_C = (2, 3, 8, 9, 64, 65, 130)
SOFTMAX_B = (1, 257)
JRC_B = (1, 2, 64, 65, 300, 1025)
# sorted sessions whose heads fall on lane 63 and lane 0 of a wave, that end on a wave boundary, span 2 to 5 waves and a workgroup
# boundary, and whose end the kernel's binary search finds inside the array and at its end (tests/test_losses.py asserts each)
JRC_PLACED_SIZES = (63, 1, 64, 65, 127, 1, 128, 63, 129, 1, 1, 62, 256, 257, 3)
SATURATED_X = (17.0, -17.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4, 0.0, -0.0, 1e-30, 3e38, -3e38)


def pointwise_inputs(B: int, scale: float, seed: int = 0):
    """float32 logits, int64 0/1 labels, float32 regression targets"""
    g = torch.Generator().manual_seed(1000 * B + int(scale) + seed)
    x = (torch.randn(B, generator=g) * scale).float()
    y = (torch.rand(B, generator=g) < 0.3).to(torch.int64)
    t = torch.randn(B, generator=g).float()
    return x, y, t


def softmax_inputs(B: int, C: int, seed: int = 0):
    g = torch.Generator().manual_seed(7000 * B + C + seed)
    return (torch.randn(B, C, generator=g) * 3).float(), torch.randint(0, C, (B,), generator=g)


def jrc_inputs(B: int, sessions: int, scale: float = 1.0, seed: int = 0):
    """[B, 2] logits, 0/1 labels, session ids drawn from `sessions` values (interleaved, not sorted)"""
    g = torch.Generator().manual_seed(31 * B + sessions + int(scale) + seed)
    x = (torch.randn(B, 2, generator=g) * scale).float()
    y = (torch.rand(B, generator=g) < 0.4).to(torch.int64)
    sid = torch.randint(0, sessions, (B,), generator=g) * 7919 - 3
    return x, y, sid


def jrc_placed_inputs(scale: float, shuffled: bool, sizes=JRC_PLACED_SIZES):
    """sessions of `sizes` rows with ascending ids, in sorted row order or shuffled"""
    sizes = torch.tensor(sizes)
    B = int(sizes.sum())
    x, y, _ = jrc_inputs(B, len(sizes), scale)
    sid = torch.repeat_interleave(torch.arange(len(sizes)) * 7919 - 3, sizes)
    if shuffled:
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(B + int(scale)))
        sid = sid[perm]
    return x, y, sid


def masked_softmax_inputs(B: int, C: int, seed: int = 0):
    """(logits, labels, mask): softmax_inputs with classes masked out by -inf, at least one per row and never the label's; for C > 64
    also class 64 + row % (C - 64), which a lane of the wave kernel meets on its second trip; row 0's only unmasked class is its label"""
    x, y = softmax_inputs(B, C, seed)
    g = torch.Generator().manual_seed(99 * B + C + seed)
    mask = torch.rand(B, C, generator=g) < 0.3
    rows = torch.arange(B)
    mask[rows, (y + 1 + rows % (C - 1)) % C] = True
    if C > 64:
        mask[rows, 64 + rows % (C - 64)] = True
    mask[0] = True
    mask[rows, y] = False
    return x.masked_fill(mask, float("-inf")), y, mask


def weight_inputs(B: int, seed: int = 0):
    """a positive weight column and an indicator label"""
    g = torch.Generator().manual_seed(555 + B + seed)
    return (torch.rand(B, generator=g) * 2 + 0.1).float(), (torch.rand(B, generator=g) < 0.5).to(torch.int64)


def row_weights(B, weight=None, space_label=None, in_w=1.0, out_w=1.0, dtype=torch.float64):
    w = torch.ones(B, dtype=dtype) if weight is None else weight.to(dtype)
    if space_label is not None:
        w = w * torch.where(space_label.to(dtype) > 0, torch.tensor(float(in_w), dtype=dtype), torch.tensor(float(out_w), dtype=dtype))
    return w


def combine(rows, w, task_weight=1.0):
    sw = w.sum()
    if float(sw) == 0.0:
        return (rows * w).sum() * 0.0
    return task_weight * (rows * w).sum() / sw


def bce_rows(x, y, label_smoothing=0.0):
    y = y.to(torch.float32)  # the reference smooths the float32 label (rank_model.py:235-239) whatever the logits' precision
    if label_smoothing > 0:
        y = y * (1.0 - label_smoothing) + 0.5 * label_smoothing
    return F.binary_cross_entropy_with_logits(x, y.to(x.dtype), reduction="none")


def focal_rows(x, y, gamma=2.0, alpha=0.5):
    y = y.to(x.dtype)
    p, omp = torch.sigmoid(x), torch.sigmoid(-x)
    f = (alpha * y * torch.pow(omp, gamma) + (1 - alpha) * (1 - y) * torch.pow(p, gamma)).detach()
    return f * F.binary_cross_entropy_with_logits(x, y, reduction="none")


def l2_rows(x, y):
    return F.mse_loss(x, y.to(x.dtype), reduction="none")


def softmax_rows(x, y, label_smoothing=0.0):
    return F.cross_entropy(x, y.long(), reduction="none", label_smoothing=label_smoothing)


def jrc_rows(x, y, sid, alpha=0.5):
    pos = y == 1
    ce = torch.logsumexp(x, dim=1) - torch.where(pos, x[:, 1], x[:, 0])
    ge = torch.zeros_like(ce)
    ninf = torch.tensor(float("-inf"), dtype=x.dtype)
    for s in torch.unique(sid):
        m = sid == s
        mp, mn = m & pos, m & ~pos
        A = torch.logsumexp(x[mn, 1], dim=0) if bool(mn.any()) else ninf
        Bs = torch.logsumexp(x[mp, 0], dim=0) if bool(mp.any()) else ninf
        z = torch.where(pos, A - x[:, 1], Bs - x[:, 0])
        ge = torch.where(m, torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs())), ge)  # (F.softplus is linear above 20)
    return alpha * ce + (1 - alpha) * ge


ROWS = {"binary_cross_entropy": bce_rows, "binary_focal_loss": focal_rows, "l2_loss": l2_rows,
        "softmax_cross_entropy": softmax_rows, "jrc_loss": jrc_rows}


def _loss_and_grad(dtype, kind, logits, labels, *args, weight=None, space_label=None, in_w=1.0, out_w=1.0, task_weight=1.0, **kw):
    x = logits.detach().to(dtype).requires_grad_(True)
    rows = ROWS[kind](x, labels, *args, **kw)
    loss = combine(rows, row_weights(x.shape[0], weight, space_label, in_w, out_w, dtype), task_weight)
    (g,) = torch.autograd.grad(loss, x, allow_unused=True)
    return loss.detach().double(), (g if g is not None else torch.zeros_like(x)).detach().double()


def loss_and_grad(kind, logits, labels, *args, **kw):
    """(loss, d loss / d logits), both float64, of float32 (or float64) logits"""
    return _loss_and_grad(torch.float64, kind, logits, labels, *args, **kw)


def loss_and_grad_fp32(kind, logits, labels, *args, **kw):
    """the fp32 literal form: the same ROWS[kind] expression and the same weight combination on float32 tensors, with autograd
    (returned as float64): what a kernel's distance to `loss_and_grad` is measured against"""
    return _loss_and_grad(torch.float32, kind, logits, labels, *args, **kw)
