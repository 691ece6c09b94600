"""SegLoss: cross-entropy with a focal exponent, plus a soft Dice term -- the usual answers to the class imbalance
of road scenes.

Over the valid pixels V = {p : y_p != ignore_index}, with s_p = softmax(z_p) over the C classes, pt_p = s_p[y_p] and
w = weight (all ones when None):

    F    = sum_V w[y_p] (1 - pt_p)^gamma (-log pt_p) / sum_V w[y_p]
    I_c  = sum_V s_p[c] [y_p = c],   S_c = sum_V s_p[c],   T_c = sum_V [y_p = c]
    d_c  = (2 I_c + dice_smooth) / (S_c + T_c + dice_smooth),   m_c = [T_c > 0],   M = sum_c m_c
    Dice = sum_c m_c (1 - d_c) / max(M, 1)
    loss = ce F + dice Dice

With gamma = 0, F is nn.CrossEntropyLoss(weight, ignore_index=..., label_smoothing=...) exactly; 0/0 is NaN, as aten.
The Dice sums run over the whole batch, classes absent from it are left out, and the class weights do not enter
them.  A term whose coefficient is 0 is left out of the loss (its NaN on a batch without valid pixels included).

`SegLoss.forward` is this definition in torch ops: the CPU path, the path of any model without `forward_loss`, and
the reference the fused kernels (csrc/loss.hip: seg_sl_*) are tested against.  On a seg_amd model on the GPU,
seg_amd.train.compute_loss / validate recognise the criterion (fused_loss_options) and never build the
full-resolution logits.

OhemCELoss (below) is cross-entropy with online hard example mining: the mean over the pixels whose loss exceeds
-log(thresh), but over no fewer than min_kept of them.  Its class docstring has the definition and the tie rule; the
fused kernels are csrc/loss.hip's seg_ohem_*.

DistillLoss (below) is pixel-wise knowledge distillation: cross-entropy plus T^2 KL(softmax(teacher / T) ||
softmax(student / T)) against a second model's logits.  Its class docstring has the definition; the fused kernels are
csrc/loss.hip's seg_kd_*.

BinarySegLoss (below) is the sigmoid loss of a one-logit model: binary cross-entropy with pos_weight and a focal
exponent, plus the foreground's soft Dice; its threshold is what validation and inference cut the logit at.  Its
class docstring has the definition; the fused kernels are csrc/loss.hip's seg_bce_*.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.nn import functional as F_


def check_seg_loss_options(ce, dice, focal_gamma, label_smoothing, dice_smooth):
    """(ce, dice, focal_gamma, dice_smooth) as floats; ValueError for what the definition excludes."""
    ce, dice, gamma, smooth, eps = (float(ce), float(dice), float(focal_gamma), float(dice_smooth),
                                    float(label_smoothing))
    for name, v in (("ce", ce), ("dice", dice), ("focal_gamma", gamma)):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if ce == 0.0 and dice == 0.0:
        raise ValueError("ce and dice must not both be 0")
    if not (math.isfinite(smooth) and smooth > 0.0):
        raise ValueError(f"dice_smooth must be a finite number > 0, got {smooth!r}")
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing!r}")
    if eps > 0.0 and gamma > 0.0:
        raise ValueError("label_smoothing > 0 together with focal_gamma > 0 is not defined")
    return ce, dice, gamma, smooth


def seg_loss_terms(logits, target, ce=1.0, dice=0.0, focal_gamma=0.0, weight=None, ignore_index=-100,
                   label_smoothing=0.0, dice_smooth=1.0):
    """(loss, F, Dice) of the module docstring for NCHW `logits` and class-index `target` [N, H, W], in torch ops.
    A term whose coefficient is 0 is not evaluated and comes back as None."""
    ce, dice, gamma, smooth = check_seg_loss_options(ce, dice, focal_gamma, label_smoothing, dice_smooth)
    C = logits.shape[1]
    valid = target != ignore_index
    if bool((valid & ((target < 0) | (target >= C))).any()):
        raise IndexError("Target out of bounds: label(s) outside [0, num_classes) that are not ignore_index")
    if weight is not None:
        weight = weight.to(logits.dtype)
    focal = soft = None
    if gamma > 0.0 or dice > 0.0:
        y = torch.where(valid, target, torch.zeros_like(target)).unsqueeze(1)        # [N, 1, H, W], ignored -> 0
        onehot = torch.zeros_like(logits, dtype=torch.bool).scatter_(1, y, True)     # [N, C, H, W]
        s = torch.softmax(logits, 1)
    if ce > 0.0:
        if gamma == 0.0:
            focal = F_.cross_entropy(logits, target, weight, ignore_index=ignore_index, reduction="mean",
                                     label_smoothing=label_smoothing)
        else:
            nlp = -torch.log_softmax(logits, 1).gather(1, y).squeeze(1)              # -log pt
            omp = s.masked_fill(onehot, 0.0).sum(1)                                  # 1 - pt as sum_{c != y} s_c
            pw = torch.where(omp > 0, torch.where(omp > 0, omp, torch.ones_like(omp)).pow(gamma),
                             torch.zeros_like(omp))                                  # exactly 0 where 1 - pt is 0
            wy = (weight[y.squeeze(1)] if weight is not None else torch.ones_like(nlp)) * valid.to(nlp.dtype)
            # where, not a product with the mask: an ignored pixel's gradient is 0 even when the quotient is 0/0
            focal = torch.where(valid, wy * pw * nlp, torch.zeros_like(nlp)).sum() / wy.sum()
    if dice > 0.0:
        vm = valid.unsqueeze(1)
        lab = onehot & vm
        sv = s * vm.to(s.dtype)
        I = (sv * lab.to(s.dtype)).sum((0, 2, 3))
        S = sv.sum((0, 2, 3))
        T = lab.sum((0, 2, 3)).to(s.dtype)
        d = (2.0 * I + smooth) / (S + T + smooth)
        m = (T > 0).to(s.dtype)
        soft = ((1.0 - d) * m).sum() / m.sum().clamp(min=1.0)
    loss = None
    for coef, term in ((ce, focal), (dice, soft)):
        if term is not None:
            loss = coef * term if loss is None else loss + coef * term
    return loss, focal, soft


def check_ohem_options(thresh, min_kept, label_smoothing=0.0, reduction="mean", ce=1.0, dice=0.0, focal_gamma=0.0):
    """(thresh as a float, min_kept as an int >= 1 or a float in (0, 1]); ValueError for what OhemCELoss's
    definition excludes: label smoothing, any reduction but the mean, SegLoss's terms."""
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or not 0.0 < float(thresh) < 1.0:
        raise ValueError(f"thresh must be a probability in (0, 1), got {thresh!r}")
    if isinstance(min_kept, bool) or not isinstance(min_kept, (int, float)):
        raise ValueError(f"min_kept must be an int >= 1 (pixels) or a float in (0, 1] (a fraction), got {min_kept!r}")
    if isinstance(min_kept, int):
        if min_kept < 1:
            raise ValueError(f"min_kept as a pixel count must be >= 1, got {min_kept!r}")
    elif not 0.0 < min_kept <= 1.0:
        raise ValueError(f"min_kept as a fraction of the batch's pixels must be in (0, 1], got {min_kept!r}")
    if float(label_smoothing) != 0.0:
        raise ValueError("online hard example mining is not defined with label smoothing")
    if reduction != "mean":
        raise ValueError(f"online hard example mining is defined for reduction 'mean' only, got {reduction!r}")
    if float(ce) != 1.0 or float(dice) != 0.0 or float(focal_gamma) != 0.0:
        raise ValueError("online hard example mining does not combine with SegLoss's ce, dice or focal_gamma")
    return float(thresh), min_kept


def resolve_min_kept(min_kept, pixels: int) -> int:
    """OhemCELoss's floor as a pixel count for a batch of `pixels` = N * Ho * Wo pixels: an int as it is, a float
    as that fraction of the batch, floored and at least 1."""
    if isinstance(min_kept, int):
        return min_kept
    return max(1, int(math.floor(min_kept * pixels)))


def ohem_loss_terms(logits, target, thresh=0.7, min_kept=1 / 16, weight=None, ignore_index=-100):
    """(loss, kept, cut) of OhemCELoss for NCHW `logits` and class-index `target` [N, H, W], in torch ops: kept is
    the bool mask [N, H, W] of K and cut = min(tau, lambda) as a 0-dim tensor (tau when no pixel is valid)."""
    thresh, min_kept = check_ohem_options(thresh, min_kept)
    C = logits.shape[1]
    valid = target != ignore_index
    if bool((valid & ((target < 0) | (target >= C))).any()):
        raise IndexError("Target out of bounds: label(s) outside [0, num_classes) that are not ignore_index")
    tau = -math.log(thresh)
    y = torch.where(valid, target, torch.zeros_like(target))
    l = -torch.log_softmax(logits, 1).gather(1, y.unsqueeze(1)).squeeze(1)           # [N, H, W], unweighted
    ld = l.detach()
    nv = int(valid.sum())
    k = min(resolve_min_kept(min_kept, target.numel()), nv)
    if nv:
        lam = torch.topk(ld[valid], k, sorted=True).values[-1]                       # the k-th largest over V
        kept = valid & ((ld > tau) | (ld >= lam))                                    # a tie group at lambda whole
        cut = torch.clamp(lam, max=tau)
    else:
        kept = valid
        cut = ld.new_tensor(tau)
    wy = (weight.to(l.dtype)[y] if weight is not None else torch.ones_like(l)) * kept.to(l.dtype)
    # where, not a product with the mask: a pixel outside K has gradient exactly 0
    loss = torch.where(kept, wy * l, torch.zeros_like(l)).sum() / wy.sum()
    return loss, kept, cut


def check_distill_options(ce, kd, temperature, label_smoothing=0.0, reduction="mean", dice=0.0, focal_gamma=0.0,
                          ohem_thresh=None, ohem_min_kept=None):
    """(ce, kd, temperature) as floats; ValueError for what DistillLoss's definition excludes: kd <= 0, ce < 0,
    temperature <= 0, a non-finite one, label smoothing, any reduction but the mean, SegLoss's Dice / focal terms
    and online hard example mining."""
    ce, kd, T = float(ce), float(kd), float(temperature)
    if not (math.isfinite(kd) and kd > 0.0):
        raise ValueError(f"kd must be a finite number > 0, got {kd!r}")
    if not (math.isfinite(ce) and ce >= 0.0):
        raise ValueError(f"ce must be a finite number >= 0, got {ce!r}")
    if not (math.isfinite(T) and T > 0.0):
        raise ValueError(f"temperature must be a finite number > 0, got {T!r}")
    if float(label_smoothing) != 0.0:
        raise ValueError("distillation is not defined with label smoothing")
    if reduction != "mean":
        raise ValueError(f"distillation is defined for reduction 'mean' only, got {reduction!r}")
    if float(dice) != 0.0 or float(focal_gamma) != 0.0:
        raise ValueError("distillation does not combine with SegLoss's dice or focal_gamma")
    if ohem_thresh is not None or ohem_min_kept is not None:
        raise ValueError("distillation does not combine with online hard example mining")
    return ce, kd, T


def distill_loss_terms(logits, teacher_logits, target, ce=1.0, kd=1.0, temperature=2.0, weight=None,
                       ignore_index=-100, kd_ignored=True):
    """(loss, CE, KD) of DistillLoss for NCHW `logits` and `teacher_logits` [N, C, Ho, Wo] and class-index `target`
    [N, Ho, Wo], in torch ops; differentiable in `logits` only.  CE is None when ce == 0 (the term is left out)."""
    ce, kd, T = check_distill_options(ce, kd, temperature)
    if teacher_logits.shape != logits.shape:
        raise ValueError(f"teacher_logits must have the logits' shape {tuple(logits.shape)}, got "
                         f"{tuple(teacher_logits.shape)}")
    C = logits.shape[1]
    valid = target != ignore_index
    if bool((valid & ((target < 0) | (target >= C))).any()):
        raise IndexError("Target out of bounds: label(s) outside [0, num_classes) that are not ignore_index")
    if weight is not None:
        weight = weight.to(logits.dtype)
    hard = None
    if ce > 0.0:
        hard = F_.cross_entropy(logits, target, weight, ignore_index=ignore_index, reduction="mean")
    u = teacher_logits.detach().to(logits.dtype)
    logq = torch.log_softmax(u / T, 1)
    logs = torch.log_softmax(logits / T, 1)
    kl = (logq.exp() * (logq - logs)).sum(1)                                         # [N, Ho, Wo]
    if kd_ignored:
        soft = kl.sum() * (T * T) / kl.numel()
    else:
        # where, not a product with the mask: a pixel outside P has gradient exactly 0
        soft = torch.where(valid, kl, torch.zeros_like(kl)).sum() * (T * T) / valid.sum()
    loss = kd * soft if hard is None else ce * hard + kd * soft
    return loss, hard, soft


def check_binary_options(bce, dice, focal_gamma, pos_weight, dice_smooth, threshold=0.5):
    """(bce, dice, focal_gamma, pos_weight, dice_smooth, threshold) as floats; ValueError for what BinarySegLoss's
    definition excludes."""
    bce, dice, gamma, pw, smooth, thr = (float(bce), float(dice), float(focal_gamma), float(pos_weight),
                                         float(dice_smooth), float(threshold))
    for name, v in (("bce", bce), ("dice", dice), ("focal_gamma", gamma)):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if bce == 0.0 and dice == 0.0:
        raise ValueError("bce and dice must not both be 0")
    if not (math.isfinite(pw) and pw > 0.0):
        raise ValueError(f"pos_weight must be a finite number > 0, got {pw!r}")
    if not (math.isfinite(smooth) and smooth > 0.0):
        raise ValueError(f"dice_smooth must be a finite number > 0, got {smooth!r}")
    if not 0.0 < thr < 1.0:
        raise ValueError(f"threshold must be a probability in (0, 1), got {thr!r}")
    return bce, dice, gamma, pw, smooth, thr


def check_binary_combination(weight=None, label_smoothing=0.0, reduction="mean", ohem_thresh=None,
                             ohem_min_kept=None, kd=0.0):
    """ValueError for what binary=True does not combine with: class weights (pos_weight is the binary loss's),
    label smoothing, any reduction but the mean, online hard example mining and distillation."""
    if weight is not None:
        raise ValueError("binary=True takes pos_weight, not class weights")
    if float(label_smoothing) != 0.0:
        raise ValueError("binary=True is not defined with label smoothing")
    if reduction != "mean":
        raise ValueError(f"binary=True is defined for reduction 'mean' only, got {reduction!r}")
    if ohem_thresh is not None or ohem_min_kept is not None:
        raise ValueError("binary=True does not combine with online hard example mining")
    if float(kd) != 0.0:
        raise ValueError("binary=True does not combine with distillation")


def logit_threshold(threshold: float) -> float:
    """zthr = log(threshold / (1 - threshold)) in float64, cast to float32: the prediction is 1 iff z > zthr, on the
    CPU and in the kernels (seg_bce_upsample_eval, seg_threshold_nearest) alike."""
    thr = float(threshold)
    if not 0.0 < thr < 1.0:
        raise ValueError(f"threshold must be a probability in (0, 1), got {threshold!r}")
    return float(torch.tensor(math.log(thr / (1.0 - thr)), dtype=torch.float64).to(torch.float32))


def binary_target(logits, target):
    """BinarySegLoss's target as an int64 [N, H, W] class-index mask: [N, 1, H, W] is squeezed, bool and the other
    integer dtypes are converted with one torch op; a floating-point target is a TypeError (soft labels are
    nn.BCEWithLogitsLoss's, on the logits path)."""
    if not isinstance(target, torch.Tensor) or target.is_floating_point() or target.is_complex():
        what = target.dtype if isinstance(target, torch.Tensor) else type(target).__name__
        raise TypeError(f"BinarySegLoss takes class-index targets (an integer or bool mask of 0 / 1 / ignore_index), "
                        f"got {what}; soft labels are nn.BCEWithLogitsLoss's")
    if target.dim() == 4 and target.shape[1] == 1:
        target = target[:, 0]
    if target.dtype != torch.int64:
        target = target.to(torch.int64)
    return target


def binary_loss_terms(logits, target, bce=1.0, dice=0.0, focal_gamma=0.0, pos_weight=1.0, ignore_index=-100,
                      dice_smooth=1.0):
    """(loss, F, Dice) of BinarySegLoss for `logits` [N, 1, H, W] and a class-index `target` [N, H, W] or
    [N, 1, H, W] with values in {0, 1, ignore_index}, in torch ops.  A term whose coefficient is 0 is not evaluated
    and comes back as None."""
    bce, dice, gamma, pw, smooth, _ = check_binary_options(bce, dice, focal_gamma, pos_weight, dice_smooth)
    if logits.dim() != 4 or logits.shape[1] != 1:
        raise ValueError(f"BinarySegLoss takes one-channel logits [N, 1, H, W], got {tuple(logits.shape)}")
    target = binary_target(logits, target)
    z = logits[:, 0]
    if target.shape != z.shape:
        raise ValueError(f"target must be [N, H, W] or [N, 1, H, W] matching the logits {tuple(logits.shape)}, got "
                         f"{tuple(target.shape)}")
    valid = target != ignore_index
    if bool((valid & ((target < 0) | (target > 1))).any()):
        raise IndexError("Target out of bounds: label(s) outside {0, 1} that are not ignore_index")
    fg = valid & (target == 1)
    vf = valid.to(z.dtype)
    focal = soft = None
    if bce > 0.0:
        x = torch.where(fg, z, -z)                                   # pt = sigmoid(x)
        nlp = F_.softplus(-x)                                        # -log pt = max(-x, 0) + log1p(exp(-|x|))
        wy = torch.where(fg, torch.full_like(z, pw), torch.ones_like(z))
        term = wy * nlp
        if gamma > 0.0:
            omp = torch.sigmoid(-x)                                  # 1 - pt
            pos = omp > 0
            term = term * torch.where(pos, torch.where(pos, omp, torch.ones_like(omp)).pow(gamma),
                                      torch.zeros_like(omp))         # exactly 0 where 1 - pt is 0
        # where, not a product with the mask: an ignored pixel's gradient is exactly 0
        focal = torch.where(valid, term, torch.zeros_like(term)).sum() / vf.sum()
    if dice > 0.0:
        s = torch.where(valid, torch.sigmoid(z), torch.zeros_like(z))
        I = torch.where(fg, s, torch.zeros_like(s)).sum()
        U = s.sum() + fg.to(z.dtype).sum() + smooth
        soft = 1.0 - (2.0 * I + smooth) / U
    loss = None
    for coef, t in ((bce, focal), (dice, soft)):
        if t is not None:
            loss = coef * t if loss is None else loss + coef * t
    return loss, focal, soft


def criterion_loss(logits, target, ignore_index=-100, weight=None, label_smoothing=0.0, reduction="mean", ce=1.0,
                   dice=0.0, focal_gamma=0.0, dice_smooth=1.0, ohem_thresh=None, ohem_min_kept=None, binary=False,
                   pos_weight=1.0):
    """What model.forward_loss's keyword arguments describe, on full-resolution logits in torch ops: F.cross_entropy
    for the defaults (nn.CrossEntropyLoss's options), else SegLoss's definition (reduction "mean" only), or
    OhemCELoss's when ohem_thresh / ohem_min_kept are given, or BinarySegLoss's with binary=True (ce is then its bce
    coefficient)."""
    if binary:
        check_binary_combination(weight, label_smoothing, reduction, ohem_thresh, ohem_min_kept)
        return binary_loss_terms(logits, target, ce, dice, focal_gamma, pos_weight, ignore_index, dice_smooth)[0]
    if ohem_thresh is not None or ohem_min_kept is not None:
        thresh, min_kept = check_ohem_options(ohem_thresh, ohem_min_kept, label_smoothing, reduction, ce, dice,
                                              focal_gamma)
        return ohem_loss_terms(logits, target, thresh, min_kept, weight, ignore_index)[0]
    if float(ce) == 1.0 and float(dice) == 0.0 and float(focal_gamma) == 0.0:
        return F_.cross_entropy(logits, target, weight, ignore_index=ignore_index, reduction=reduction,
                                label_smoothing=label_smoothing)
    if reduction != "mean":
        raise ValueError(f"a Dice or focal term (or ce != 1) is defined for reduction 'mean' only, got {reduction!r}")
    return seg_loss_terms(logits, target, ce, dice, focal_gamma, weight, ignore_index, label_smoothing,
                          dice_smooth)[0]


class SegLoss(nn.Module):
    """loss = ce * F + dice * Dice (module docstring): weighted cross-entropy with label smoothing (focal_gamma = 0)
    or its focal form (focal_gamma > 0), plus a soft Dice term over the batch.  The reduction is always the mean.

    Under seg_amd.ddp.DataParallel the Dice sums are per rank, like BatchNorm statistics."""

    def __init__(self, ce: float = 1.0, dice: float = 0.0, focal_gamma: float = 0.0, weight=None,
                 ignore_index: int = -100, label_smoothing: float = 0.0, dice_smooth: float = 1.0):
        super().__init__()
        self.ce, self.dice, self.focal_gamma, self.dice_smooth = check_seg_loss_options(
            ce, dice, focal_gamma, label_smoothing, dice_smooth)
        self.ignore_index = int(ignore_index)
        self.label_smoothing = float(label_smoothing)
        self.register_buffer("weight", weight)

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return seg_loss_terms(logits, target, self.ce, self.dice, self.focal_gamma, self.weight, self.ignore_index,
                              self.label_smoothing, self.dice_smooth)[0]

    def extra_repr(self) -> str:
        return (f"ce={self.ce}, dice={self.dice}, focal_gamma={self.focal_gamma}, ignore_index={self.ignore_index}, "
                f"label_smoothing={self.label_smoothing}, dice_smooth={self.dice_smooth}")


class BinarySegLoss(nn.Module):
    """The sigmoid loss of a one-logit model (lanes, road: MobileNetV2UNet(1), UNet(1), LightUNet):
    loss = bce * F + dice * Dice, binary cross-entropy with pos_weight and a focal exponent plus the soft Dice of the
    foreground.

    Logits are [N, 1, H, W]; targets are class-index masks [N, H, W] or [N, 1, H, W] with values in {0, 1,
    ignore_index}, of an integer or bool dtype (anything but int64 is converted with one torch op; a floating-point
    target is a TypeError -- soft labels are nn.BCEWithLogitsLoss's business).  Over the valid pixels
    V = {p : y_p != ignore_index}, with z_p the pixel's logit, t_p = y_p, w_p = pos_weight where t_p = 1 else 1 and
    pt_p = sigmoid(z_p) where t_p = 1 else sigmoid(-z_p):

        F    = sum_V w_p (1 - pt_p)^gamma (-log pt_p) / |V|
        I = sum_V sigmoid(z_p) t_p,   S = sum_V sigmoid(z_p),   T = sum_V t_p,   U = S + T + dice_smooth
        Dice = 1 - (2 I + dice_smooth) / U
        loss = bce F + dice Dice

    The divisor of F is |V|, not sum w: with gamma = 0 and nothing ignored F is exactly
    nn.BCEWithLogitsLoss(pos_weight=torch.tensor(pos_weight))(z, t.float()).  A term whose coefficient is 0 is left
    out (its NaN included); no valid pixel gives NaN (0/0, as aten); (1 - pt)^gamma is exactly 0 where 1 - pt rounds
    to 0.  The Dice term is over the foreground only and over the whole batch -- per rank under
    seg_amd.ddp.DataParallel, as SegLoss's.  A label outside {0, 1} that is not ignore_index raises IndexError.

    threshold belongs to validation and inference only: the prediction is 1 iff z > log(threshold / (1 - threshold))
    (logit_threshold: formed in float64, cast to float).  The comparison is strict, so a tie or a NaN logit is
    background -- "first maximum wins" for the two-class view [0, z].

    `forward` is this definition in torch ops: the CPU path, the path of any model without `forward_loss`, and the
    reference the fused kernels (csrc/loss.hip: seg_bce_*) are tested against.  On a seg_amd model on the GPU,
    seg_amd.train.compute_loss / validate recognise the criterion (fused_loss_options) and never build the
    full-resolution logits or their gradient."""

    def __init__(self, bce: float = 1.0, dice: float = 0.0, focal_gamma: float = 0.0, pos_weight: float = 1.0,
                 ignore_index: int = -100, dice_smooth: float = 1.0, threshold: float = 0.5):
        super().__init__()
        (self.bce, self.dice, self.focal_gamma, self.pos_weight, self.dice_smooth,
         self.threshold) = check_binary_options(bce, dice, focal_gamma, pos_weight, dice_smooth, threshold)
        self.ignore_index = int(ignore_index)

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return binary_loss_terms(logits, target, self.bce, self.dice, self.focal_gamma, self.pos_weight,
                                 self.ignore_index, self.dice_smooth)[0]

    def extra_repr(self) -> str:
        return (f"bce={self.bce}, dice={self.dice}, focal_gamma={self.focal_gamma}, pos_weight={self.pos_weight}, "
                f"ignore_index={self.ignore_index}, dice_smooth={self.dice_smooth}, threshold={self.threshold}")


class OhemCELoss(nn.Module):
    """Cross-entropy with online hard example mining: the mean over the pixels the model still gets wrong, but never
    over fewer than a floor (BiSeNet's OhemCELoss(thresh, n_min) is OhemCELoss(thresh, min_kept=n_min)).

    Over the valid pixels V = {p : y_p != ignore_index} of the whole batch, with l_p = logsumexp(z_p) - z_p[y_p] the
    unweighted cross-entropy, w = weight (all ones when None), tau = -log(thresh) and k = min(min_kept, |V|):

        lambda = the k-th largest l_p over V
        K      = {p in V : l_p > tau or l_p >= lambda}
        loss   = sum_K w[y_p] l_p / sum_K w[y_p]

    min_kept: an int >= 1 is a pixel count per batch; a float in (0, 1] is that fraction of the batch's N * Ho * Wo
    pixels, floored and at least 1 (resolved when the shape is known).  The gradient treats K as a constant, as
    indexing does: it is exactly 0 outside K.  No valid pixel gives NaN (0/0, as aten).

    Ties: every pixel whose loss equals lambda is kept, so |K| can exceed k where `loss.topk(k)` would keep an
    arbitrary k of them; K then depends on neither the pixel order nor a kernel's thread mapping.  Without ties at
    lambda the value is BiSeNet's (`loss[loss > tau]`, or `loss.topk(n_min)` when fewer than n_min pass).

    `forward` is this definition in torch ops: the CPU path, the path of any model without `forward_loss`, and the
    reference the fused kernels (csrc/loss.hip: seg_ohem_*) are tested against.  On a seg_amd model on the GPU,
    seg_amd.train.compute_loss / validate recognise the criterion (fused_loss_options) and never build the
    full-resolution logits.

    Under seg_amd.ddp.DataParallel the selection is per rank (each rank mines its own shard of the batch), like
    SegLoss's Dice sums and the BatchNorm statistics."""

    def __init__(self, thresh: float = 0.7, min_kept=1 / 16, weight=None, ignore_index: int = -100):
        super().__init__()
        self.thresh, self.min_kept = check_ohem_options(thresh, min_kept)
        self.ignore_index = int(ignore_index)
        self.register_buffer("weight", weight)

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ohem_loss_terms(logits, target, self.thresh, self.min_kept, self.weight, self.ignore_index)[0]

    def extra_repr(self) -> str:
        return f"thresh={self.thresh}, min_kept={self.min_kept}, ignore_index={self.ignore_index}"


class DistillLoss(nn.Module):
    """Pixel-wise knowledge distillation: hard-label cross-entropy plus the tempered KL divergence to a teacher.

    Over the valid pixels V = {p : y_p != ignore_index} and the distilled pixels P (every pixel with kd_ignored=True
    -- the teacher also supervises unlabelled regions -- else V), with z_p the student's logits, u_p the teacher's,
    T the temperature, s = softmax(z_p / T), q = softmax(u_p / T) and w = weight (all ones when None):

        CE   = sum_V w[y_p] (logsumexp(z_p) - z_p[y_p]) / sum_V w[y_p]     (nn.CrossEntropyLoss(weight, ignore_index))
        KD   = T^2 / |P| sum_P sum_c q_c (log q_c - log s_c)
        loss = ce CE + kd KD

    A term whose coefficient is 0 is left out, so ce = 0 on a batch without valid pixels is not NaN.  The teacher
    gets no gradient.  Label smoothing, reductions other than the mean, Dice / focal terms and online hard example
    mining are not combined with distillation (ValueError).

    `teacher` is held but NOT registered as a submodule: the criterion's parameters(), state_dict() and .to() do not
    include it, so no checkpoint of the student contains the teacher's weights; move the teacher to the device
    yourself.  The constructor puts it in eval mode and clears requires_grad on its parameters; using the criterion
    while the teacher is in training mode raises.

    `forward(logits, target, teacher_logits)` is the definition in torch ops on full-resolution logits: the CPU
    path, the path of any model without `forward_loss`, and the reference the fused kernels (csrc/loss.hip:
    seg_kd_*) are tested against.  On seg_amd models on the GPU, seg_amd.train.compute_loss recognises the criterion
    (fused_loss_options), asks the teacher for its low-resolution logits (forward_low_logits) and never builds
    either model's full-resolution logits.  validate() evaluates hard(): validation does not distil.

    Under seg_amd.ddp.DataParallel every rank distils its own shard; the gradients are averaged."""

    def __init__(self, teacher: nn.Module, ce: float = 1.0, kd: float = 1.0, temperature: float = 2.0, weight=None,
                 ignore_index: int = -100, kd_ignored: bool = True):
        super().__init__()
        self.ce, self.kd, self.temperature = check_distill_options(ce, kd, temperature)
        self.ignore_index = int(ignore_index)
        self.kd_ignored = bool(kd_ignored)
        self.register_buffer("weight", weight)
        if not isinstance(teacher, nn.Module):
            raise TypeError(f"teacher must be an nn.Module, got {type(teacher).__name__}")
        teacher.eval()
        teacher.requires_grad_(False)
        object.__setattr__(self, "teacher", teacher)  # not a submodule: see the class docstring

    def _check_teacher(self):
        if self.teacher.training:
            raise RuntimeError("DistillLoss: the teacher is in training mode; call teacher.eval() (its BatchNorm "
                               "statistics must not follow the student's batches)")

    def forward(self, logits: torch.Tensor, target: torch.Tensor, teacher_logits: torch.Tensor) -> torch.Tensor:
        self._check_teacher()
        return distill_loss_terms(logits, teacher_logits, target, self.ce, self.kd, self.temperature, self.weight,
                                  self.ignore_index, self.kd_ignored)[0]

    def teacher_logits(self, x: torch.Tensor) -> torch.Tensor:
        """The teacher's full-resolution logits for the batch `x`, without gradients."""
        self._check_teacher()
        with torch.no_grad():
            return self.teacher(x)

    def hard(self) -> nn.CrossEntropyLoss:
        """The criterion's cross-entropy term as a criterion of its own (what validate() evaluates)."""
        return nn.CrossEntropyLoss(self.weight, ignore_index=self.ignore_index)

    def extra_repr(self) -> str:
        return (f"teacher={type(self.teacher).__name__}, ce={self.ce}, kd={self.kd}, "
                f"temperature={self.temperature}, ignore_index={self.ignore_index}, kd_ignored={self.kd_ignored}")
