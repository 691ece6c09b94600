"""Segmentation metrics from a confusion matrix (row = label, column = predicted class).

The reference has no metric code (its validation block, src/train.py:46-76, is commented
out); the definitions are the ones seg_amd.detinit.miou fixes: IoU_c = TP / (TP + FP + FN),
mIoU = the mean over the classes whose union is not empty.

On the MI355X the matrix is filled by the fused validation kernel
(`model.forward_metrics`, csrc/loss.hip: seg_ce_upsample_eval) and stays on the device for
a whole pass; `summarize` is the one place it comes to the host.
"""
from __future__ import annotations

import torch


def add_confusion(confusion: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, ignore_index: int = -100) -> None:
    """confusion[label, pred] += 1 (in place, on confusion's device) for every pixel whose label is
    neither ignore_index nor outside [0, C) -- the torch composition of what the fused kernel
    counts, for CPU tensors and for criteria or models the fused path does not cover."""
    C = confusion.shape[0]
    t = target.reshape(-1)
    p = pred.reshape(-1)
    keep = (t != ignore_index) & (t >= 0) & (t < C)
    idx = t[keep] * C + p[keep]
    confusion += torch.bincount(idx, minlength=C * C).reshape(C, C).to(confusion.dtype)


def summarize(confusion: torch.Tensor) -> dict:
    """{"confusion": int64 CPU [C, C], "pixel_acc": float, "iou": float64 CPU [C] (NaN where the
    class's union is empty), "miou": float (mean over the non-empty unions; NaN if there is none)}."""
    cm = confusion.detach().to("cpu", torch.int64)
    d = cm.double()
    tp = d.diag()
    union = d.sum(0) + d.sum(1) - tp
    valid = union > 0
    iou = torch.full_like(tp, float("nan"))
    iou[valid] = tp[valid] / union[valid]
    total = d.sum()
    return {"confusion": cm,
            "pixel_acc": float(tp.sum() / total) if total > 0 else float("nan"),
            "iou": iou,
            "miou": float(iou[valid].mean()) if valid.any() else float("nan")}


def binary_summary(confusion: torch.Tensor) -> dict:
    """{"precision", "recall", "f1"} of class 1 from a [2, 2] confusion matrix (row = label, column = prediction):
    TP / (TP + FP), TP / (TP + FN) and 2 TP / (2 TP + FP + FN), each NaN where its denominator is 0."""
    cm = confusion.detach().to("cpu", torch.int64)
    if tuple(cm.shape) != (2, 2):
        raise ValueError(f"binary_summary takes a [2, 2] confusion matrix, got {tuple(cm.shape)}")
    tp, fp, fn = int(cm[1, 1]), int(cm[0, 1]), int(cm[1, 0])

    def ratio(num, den):
        return num / den if den > 0 else float("nan")

    return {"precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn), "f1": ratio(2 * tp, 2 * tp + fp + fn)}


def class_weights(counts, scheme: str = "median_frequency", clip: float | None = None) -> torch.Tensor:
    """Class weights for nn.CrossEntropyLoss(weight=...) from pixel counts: a float32 CPU [C] tensor.

    counts: a length-C vector of label pixel counts, or a [C, C] confusion matrix (row = label), whose
    row sums are those counts -- validate()["confusion"] as it stands.
    scheme: "median_frequency": w_c = median(n) / n_c, the median taken over the classes that occur
    (the lower one of an even number, so the class at the median gets exactly 1.0);
    "inverse": w_c = sum(n) / (#classes that occur * n_c), which averages to 1 over the pixels.
    A class that never occurs gets weight 0.  clip: an upper bound applied last."""
    n = torch.as_tensor(counts).detach().to("cpu", torch.float64)
    if n.dim() == 2 and n.shape[0] == n.shape[1]:
        n = n.sum(1)
    if n.dim() != 1 or n.numel() == 0 or bool((n < 0).any()):
        raise ValueError("counts must be a non-negative length-C vector or a [C, C] confusion matrix")
    present = n > 0
    w = torch.zeros_like(n)
    if present.any():
        if scheme == "median_frequency":
            w[present] = n[present].median() / n[present]
        elif scheme == "inverse":
            w[present] = n.sum() / (int(present.sum()) * n[present])
        else:
            raise ValueError(f"scheme must be 'median_frequency' or 'inverse', got {scheme!r}")
    elif scheme not in ("median_frequency", "inverse"):
        raise ValueError(f"scheme must be 'median_frequency' or 'inverse', got {scheme!r}")
    if clip is not None:
        w = w.clamp(max=float(clip))
    return w.to(torch.float32)
