"""Pure-torch float64 restatement of the evaluation metrics (torchmetrics is not installed): what tests/test_eval_*.py
compare `torcheasyrec_amd.metrics` against.

Assumptions, each the reference's definition:
* binned AUROC (torchmetrics' binary form with a thresholds tensor, tzrec/metrics/decay_auc.py:42-60): a sample is predicted
  positive at threshold t iff `pred >= thresholds[t]` (a float32 comparison, broadcast [B, T]); confmat[t] = [[tn, fp], [fn, tp]];
  tpr = tp / (tp + fn), fpr = fp / (fp + tn) with 0 / 0 = 0, both flipped, integrated by trapezoid in float64.
* normalized entropy (tzrec/metrics/normalized_entropy.py): sum of F.binary_cross_entropy (each log clamped at -100) over
  -(pos log m + neg log(1 - m)), m = pos / n clamped to [eta, 1 - eta]; here with float64 logs of the float32 predictions.
* grouped AUC (tzrec/metrics/grouped_auc.py:96-125): mean over the groups that hold both classes of the group's exact
  AUROC = the share of (positive, negative) pairs ranked correctly, a tied pair counting one half -- computed pairwise, O(n^2).
"""
import torch


def bins(preds: torch.Tensor, thresholds: torch.Tensor) -> torch.Tensor:
    """number of thresholds <= pred, per sample"""
    return (preds[:, None] >= thresholds[None, :]).sum(dim=1)


def bins_sorted(preds: torch.Tensor, thresholds: torch.Tensor) -> torch.Tensor:
    """`bins` without the [B, T] mask, for ascending thresholds: a binary search per sample (a NaN compares false: bin 0)"""
    b = torch.searchsorted(thresholds, preds.contiguous(), right=True)
    return torch.where(torch.isnan(preds), torch.zeros_like(b), b)


def histogram(preds, target, thresholds, bins_of=bins) -> torch.Tensor:
    """int64 [T + 1, 2]: samples per (bin, class)"""
    T = thresholds.numel()
    flat = bins_of(preds, thresholds) * 2 + (target != 0).to(torch.int64)
    return torch.bincount(flat, minlength=(T + 1) * 2).view(T + 1, 2)


def confmat(preds, target, thresholds) -> torch.Tensor:
    """int64 [T, 2, 2] indexed [threshold, target, prediction]"""
    pred_pos = preds[:, None] >= thresholds[None, :]  # [B, T]
    pos = (target != 0)[:, None]
    tp, fp = (pred_pos & pos).sum(0), (pred_pos & ~pos).sum(0)
    fn, tn = (~pred_pos & pos).sum(0), (~pred_pos & ~pos).sum(0)
    return torch.stack([torch.stack([tn, fp], 1), torch.stack([fn, tp], 1)], 1).to(torch.int64)


def auc_from_confmat(c: torch.Tensor) -> torch.Tensor:
    c = c.to(torch.float64)
    tp, fp, fn, tn = c[:, 1, 1], c[:, 0, 1], c[:, 1, 0], c[:, 0, 0]
    tpr = torch.where(tp + fn > 0, tp / (tp + fn), torch.zeros_like(tp)).flip(0)
    fpr = torch.where(fp + tn > 0, fp / (fp + tn), torch.zeros_like(fp)).flip(0)
    return torch.trapz(tpr, fpr)


def normalized_entropy(preds, target, eta: float = 1e-12) -> torch.Tensor:
    p, y = preds.to(torch.float64), (target != 0).to(torch.float64)
    ce = -(y * torch.log(p).clamp(min=-100.0) + (1.0 - y) * torch.log1p(-p).clamp(min=-100.0))
    n, pos = float(y.numel()), y.sum()
    m = (pos / n).clamp(eta, 1.0 - eta)
    return ce.sum() / -(pos * torch.log(m) + (n - pos) * torch.log(1.0 - m))


def grouped_auc_parts(preds, target, keys):
    """(sum of the counted groups' AUCs as float64, number of counted groups)"""
    total, counted = 0.0, 0
    for k in torch.unique(keys).tolist():
        sel = keys == k
        p, y = preds[sel], target[sel] != 0
        pp, nn = p[y], p[~y]
        if pp.numel() == 0 or nn.numel() == 0:
            continue
        wins = (pp[:, None] > nn[None, :]).sum().item() + 0.5 * (pp[:, None] == nn[None, :]).sum().item()
        total += wins / (pp.numel() * nn.numel())
        counted += 1
    return total, counted


def grouped_auc(preds, target, keys) -> float:
    total, counted = grouped_auc_parts(preds, target, keys)
    return total / counted
