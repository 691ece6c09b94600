"""Drop-in replacements for the reference's src/unet.py models.

Same class names, constructor arguments, sub-module attribute names and
state_dict keys as the reference (src/unet.py:7-171), so that
`MobileNetV2UNet(output_channels=10).to(device)` (main.py:98, inference.py:23),
`model.load_state_dict(torch.load(...))` (inference.py:24, convert.py:23) and
`torch.save(model.state_dict(), ...)` (src/train.py:77) work unchanged.

The modules hold parameters/buffers only.  `forward` runs the whole network
on the MI355X HIP kernels (seg_amd/engine.py) as one autograd node: NHWC
activations, fused BN/activation/residual, virtual skip-concat, and a backward
pass that is the engine's own reverse program.  GPU input never falls back to
anything else; CPU input (the reference's CPU device, main.py:13-21) runs the
reference composition in torch ops (seg_amd/export.py) for that device only.
"""
from __future__ import annotations

import torch
from torch import nn

from .mobilenet import MobileNetV2, load_backbone_weights


class double_conv(nn.Module):
    """(conv3x3(+bias) => BN => ReLU) * 2  -- src/unet.py:53-68"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True),
            nn.Conv2d(out_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True))


class inconv(nn.Module):
    """src/unet.py:71-77"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = double_conv(in_ch, out_ch)


class down(nn.Module):
    """MaxPool2d(2) + double_conv -- src/unet.py:80-91"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.mpconv = nn.Sequential(nn.MaxPool2d(2), double_conv(in_ch, out_ch))


class up(nn.Module):
    """bilinear x2 (align_corners=False) of x1, cat([x2, x1]), double_conv -- src/unet.py:94-105"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.up = nn.Upsample(scale_factor=2, mode="bilinear")
        self.conv = double_conv(in_ch, out_ch)


class outconv(nn.Module):
    """1x1 -> BN -> ReLU -> 1x1 head -- src/unet.py:108-121"""

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = nn.Sequential(
            nn.Conv2d(in_ch, in_ch // 2, 1), nn.BatchNorm2d(in_ch // 2), nn.ReLU(inplace=True),
            nn.Conv2d(in_ch // 2, out_ch, 1))


class _SegModel(nn.Module):
    """Shared forward.  A CUDA tensor runs through the HIP engine (and nothing else: a
    missing libsegamd.so raises).  A CPU tensor -- main.py:13-21 picks the CPU when no GPU
    is present, BASELINE configs[0] -- runs the reference's own composition in torch ops
    on this module's parameters (seg_amd.export.torch_forward), so train_model, Adam and
    state_dict work there too; the product never selects it for GPU input."""

    def train(self, mode: bool = True):
        """nn.Module.train, after which the BatchNorm layers frozen by seg_amd.freeze(bn_stats=True) are back in
        eval mode: a training loop's model.train() keeps the freeze."""
        super().train(mode)
        from .freeze import keep_frozen
        keep_frozen(self)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.device.type == "cpu":
            from .export import torch_forward
            return torch_forward(self, x)
        from .engine import run_logits
        return run_logits(self, x)

    def forward_loss(self, x: torch.Tensor, target: torch.Tensor, ignore_index: int = -100, weight=None,
                     label_smoothing: float = 0.0, reduction: str = "mean", *, ce: float = 1.0, dice: float = 0.0,
                     focal_gamma: float = 0.0, dice_smooth: float = 1.0, ohem_thresh=None,
                     ohem_min_kept=None, kd: float = 0.0, kd_temperature: float = 1.0, kd_ignored: bool = True,
                     teacher_logits=None, binary: bool = False, pos_weight: float = 1.0) -> torch.Tensor:
        """nn.CrossEntropyLoss()(self(x), target) (main.py:99, src/train.py:37) fused
        with the final upsample: the full-resolution logits are never stored.

        weight (float32 [C] on x's device), label_smoothing (in [0, 1]) and reduction ("mean" |
        "sum") are nn.CrossEntropyLoss's for class-index targets and stay fused; anything else
        (reduction="none" included) is a ValueError.  The weight tensor is read when the kernels
        run: editing it in place or passing another one needs no new launch plan.

        ce, dice, focal_gamma and dice_smooth are seg_amd.SegLoss's (seg_amd/losses.py has the definition): the
        loss becomes ce * F + dice * Dice with the focal exponent in F, fused in the same way (reduction "mean"
        only).  ohem_thresh and ohem_min_kept are seg_amd.OhemCELoss's thresh and min_kept: given (both), the loss
        is its mean over the mined pixels, selected on the device (mean reduction, no label smoothing, none of
        SegLoss's terms).  kd, kd_temperature and kd_ignored are seg_amd.DistillLoss's kd, temperature and kd_ignored
        and teacher_logits its teacher's forward_low_logits(x): given kd > 0 (with the tensor), the loss is ce * CE +
        kd * KD against the teacher, whose logits are upsampled inside the loss kernels like the student's (mean
        reduction, class weights, nothing else; GPU tensors only -- on the CPU use the criterion itself).  The
        defaults are plain cross-entropy, on the code path it always took.

        binary=True is seg_amd.BinarySegLoss for a one-channel model: ce is then its bce coefficient, dice,
        focal_gamma and dice_smooth keep their names and pos_weight is its own (seg_bce_* kernels: neither the
        full-resolution logits nor their gradient are stored).  The target may be [N, 1, H, W] and of any integer or
        bool dtype.  Class weights, label smoothing, another reduction, OHEM and kd do not combine with it."""
        if x.device.type == "cpu":
            if kd != 0.0 or teacher_logits is not None:
                raise RuntimeError("forward_loss with kd > 0 runs on the MI355X HIP path only; on CPU tensors "
                                   "evaluate the DistillLoss on the models' logits (seg_amd.train.compute_loss does)")
            from .losses import criterion_loss
            if binary:
                return criterion_loss(self(x), target, ignore_index, weight, label_smoothing, reduction, ce, dice,
                                      focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept, True, pos_weight)
            return criterion_loss(self(x), target, ignore_index, weight, label_smoothing, reduction, ce, dice,
                                  focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept)
        from .engine import run_loss
        if binary:
            return run_loss(self, x, target, ignore_index, weight, label_smoothing, reduction, ce, dice, focal_gamma,
                            dice_smooth, ohem_thresh, ohem_min_kept, kd, kd_temperature, kd_ignored, teacher_logits,
                            True, pos_weight)
        return run_loss(self, x, target, ignore_index, weight, label_smoothing, reduction, ce, dice, focal_gamma,
                        dice_smooth, ohem_thresh, ohem_min_kept, kd, kd_temperature, kd_ignored, teacher_logits)

    def forward_low_logits(self, x: torch.Tensor) -> torch.Tensor:
        """The logits in front of the final upsample, without gradients: a float32 tensor [N, Hl, Wl, round4(C)] of
        NHWC rows (pad channels 0) that the caller owns.  No full-resolution tensor is formed.  It is what a
        seg_amd.DistillLoss's teacher feeds the student's forward_loss as teacher_logits; GPU tensors only."""
        from .engine import run_low_logits
        return run_low_logits(self, x)

    def forward_metrics(self, x: torch.Tensor, target: torch.Tensor, confusion: torch.Tensor,
                        ignore_index: int = -100, weight=None, label_smoothing: float = 0.0,
                        reduction: str = "mean", *, ce: float = 1.0, dice: float = 0.0, focal_gamma: float = 0.0,
                        dice_smooth: float = 1.0, ohem_thresh=None, ohem_min_kept=None, binary: bool = False,
                        pos_weight: float = 1.0, threshold: float = 0.5) -> torch.Tensor:
        """Validation step: returns nn.CrossEntropyLoss()(self(x), target) and adds every
        non-ignored pixel to `confusion[label, argmax(self(x))]` (int64 [C, C] on x's device, in
        place), without gradients.  On the MI355X one kernel does both from the low-resolution
        logits: the full-resolution logits are never stored.  weight, label_smoothing, reduction and
        SegLoss's ce, dice, focal_gamma, dice_smooth and OhemCELoss's ohem_thresh, ohem_min_kept (as in forward_loss)
        change the returned loss only, never the matrix.  binary=True (with pos_weight, as in forward_loss) is
        seg_amd.BinarySegLoss for a one-channel model: `confusion` is then int64 [2, 2] and the prediction is
        z > log(threshold / (1 - threshold)), strictly (seg_bce_upsample_eval)."""
        if x.device.type == "cpu":
            if binary:
                return _torch_metrics(self, x, target, confusion, ignore_index, weight, label_smoothing, reduction,
                                      ce, dice, focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept, True,
                                      pos_weight, threshold)
            return _torch_metrics(self, x, target, confusion, ignore_index, weight, label_smoothing, reduction, ce,
                                  dice, focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept)
        from .engine import run_metrics
        if binary:
            return run_metrics(self, x, target, confusion, ignore_index, weight, label_smoothing, reduction, ce,
                               dice, focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept, True, pos_weight,
                               threshold)
        return run_metrics(self, x, target, confusion, ignore_index, weight, label_smoothing, reduction, ce, dice,
                           focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept)

    def forward_tta(self, x: torch.Tensor, tta) -> torch.Tensor:
        """The class probabilities p [N, C, H, W] (float32) of a test-time-augmentation ensemble, without gradients:
        tta is a seg_amd.TTA or "hflip" (seg_amd/tta.py has the definition).  p = sum_v w_v softmax(z_v) over the
        flipped / rescaled views, every z_v taken from its view's low-resolution logits by ONE interpolation to the
        output grid.  On the MI355X each view is one forward-only pass in front of the final upsample and one kernel
        forms p (seg_tta_upsample_eval); the views' full-resolution logits are never stored."""
        if x.device.type == "cpu":
            from .tta import torch_forward_tta
            return torch_forward_tta(self, x, tta)
        from .tta import run_forward_tta
        return run_forward_tta(self, x, tta)

    def forward_metrics_tta(self, x: torch.Tensor, target: torch.Tensor, confusion: torch.Tensor, tta,
                            ignore_index: int = -100, weight=None, reduction: str = "mean") -> torch.Tensor:
        """forward_metrics on the ensemble of forward_tta: returns nn.NLLLoss(weight, ignore_index, reduction)(log p,
        target) and adds every non-ignored pixel to `confusion[label, first maximum of p]`.  Only a criterion's hard
        term has a meaning for an ensemble's report -- class weights, ignore_index, reduction "mean" | "sum"; label
        smoothing, Dice, focal and OHEM terms shape training and are not taken.  On the MI355X the loss, the argmax
        and the matrix come from one kernel (seg_tta_upsample_eval) behind the views' forwards; an out-of-range label
        makes the loss NaN and is counted for engine.bad_label_count, as in forward_metrics."""
        if x.device.type == "cpu":
            from .tta import torch_metrics_tta
            return torch_metrics_tta(self, x, target, confusion, tta, ignore_index, weight, reduction)
        from .tta import run_metrics_tta
        return run_metrics_tta(self, x, target, confusion, tta, ignore_index, weight, reduction)


@torch.no_grad()
def _torch_metrics(model, x, target, confusion, ignore_index, weight=None, label_smoothing=0.0, reduction="mean",
                   ce=1.0, dice=0.0, focal_gamma=0.0, dice_smooth=1.0, ohem_thresh=None, ohem_min_kept=None,
                   binary=False, pos_weight=1.0, threshold=0.5):
    """forward_metrics in torch ops (CPU tensors): F.cross_entropy raises on an out-of-range label by itself.
    binary: the prediction is logits[:, 0] > zthr and the matrix [2, 2]."""
    from .losses import criterion_loss
    from .metrics import add_confusion
    logits = model(x)
    if binary:
        from .losses import binary_target, logit_threshold
        target = binary_target(logits, target)
        loss = criterion_loss(logits, target, ignore_index, weight, label_smoothing, reduction, ce, dice,
                              focal_gamma, dice_smooth, ohem_thresh, ohem_min_kept, True, pos_weight)
        add_confusion(confusion, (logits[:, 0] > logit_threshold(threshold)).to(torch.int64), target, ignore_index)
        return loss
    loss = criterion_loss(logits, target, ignore_index, weight, label_smoothing, reduction, ce, dice, focal_gamma,
                          dice_smooth, ohem_thresh, ohem_min_kept)
    add_confusion(confusion, logits.argmax(1), target, ignore_index)
    return loss


class MobileNetV2UNet(_SegModel):
    """src/unet.py:7-51.  `backbone_weights`: optional LOCAL path to torchvision
    MobileNetV2 ImageNet weights (the reference downloads them, src/unet.py:12)."""

    def __init__(self, output_channels=1, backbone_weights: str | None = None):
        super().__init__()
        self.backbone = MobileNetV2()
        if backbone_weights:
            load_backbone_weights(self.backbone, backbone_weights)
        f = self.backbone.features
        self.down1 = f[:2]      # 16 ch, 1/2
        self.down2 = f[2:4]     # 24 ch, 1/4
        self.down3 = f[4:7]     # 32 ch, 1/8
        self.down4 = f[7:11]    # 64 ch, 1/16
        self.down5 = f[11:19]   # 1280 ch, 1/32
        self.up1 = up(1280 + 64, 256)
        self.up2 = up(256 + 32, 128)
        self.up3 = up(128 + 24, 64)
        self.up4 = up(64 + 16, 32)
        self.outc = outconv(32, output_channels)
        self.final_upsample = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)


class UNet(_SegModel):
    """src/unet.py:124-147"""

    def __init__(self, output_channels=1, base_filters=64):
        super().__init__()
        b = base_filters
        self.inc = inconv(3, b)
        self.down1 = down(b, b * 2)
        self.down2 = down(b * 2, b * 4)
        self.down3 = down(b * 4, b * 4)
        self.up1 = up(b * 8, b * 2)
        self.up2 = up(b * 4, b)
        self.up3 = up(b * 2, b)
        self.sem_out = outconv(b, output_channels)


class LightUNet(_SegModel):
    """src/unet.py:149-171 (UNet with base 32 and one output channel)."""

    def __init__(self, base_filters=32):
        super().__init__()
        b = base_filters
        self.inc = inconv(3, b)
        self.down1 = down(b, b * 2)
        self.down2 = down(b * 2, b * 4)
        self.down3 = down(b * 4, b * 4)
        self.up1 = up(b * 8, b * 2)
        self.up2 = up(b * 4, b)
        self.up3 = up(b * 2, b)
        self.sem_out = outconv(b, 1)
