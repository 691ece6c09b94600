"""Test-time augmentation: flip and multi-scale ensembles of one model's views of an image.

    tta = seg_amd.TTA(scales=(0.75, 1.0, 1.25), hflip=True)      # "hflip" is shorthand for TTA()
    p = model.forward_tta(x, tta)                                  # [N, C, H, W] class probabilities
    loss = model.forward_metrics_tta(x, target, confusion, tta)    # validation step
    seg_amd.validate(model, loader, criterion, device, tta=tta)    # ... and the loop; Predictor(..., tta=tta)

Definition.  Views, in order: for each scale the plain view, then the mirrored one when `hflip` is set (at most
MAX_VIEWS = 8).  The view of an H x W input at scale s has size Hv = d * max(1, int(H * s / d + 0.5)) (Wv likewise),
d the model's size divisor (32 for MobileNetV2UNet, 8 for UNet / LightUNet); its tensor is
flip(F.interpolate(x, (Hv, Wv), mode="bilinear", align_corners=False), -1), a scale that keeps the size doing no
resize.  View v's low-resolution logits L_v (the model's logits in front of its final upsample) are sampled at output
pixel (y, x) of the model's Ho x Wo output grid at scale 1 exactly as the final align_corners=True upsample would
sample them -- ONE interpolation from L_v's grid to the output grid, not upsample-then-resize; a mirrored view is
read at x_v = Wo - 1 - x -- giving z_v, and

    p = sum_v w_v * softmax(z_v)   (fp32),      class = the first maximum of p,

with one positive weight per scale, shared by its two views and normalised to sum 1 over all views (default: uniform).
Validation: loss = nn.NLLLoss(weight, ignore_index, reduction)(log p, target), confusion[label, class] += 1 per valid
pixel.  On the MI355X every view runs through seg_tta_view_nchw and the forward-only low-logits plan, and one
seg_tta_upsample_eval (csrc/tta.hip) does the rest: no full-resolution logits, no torch ops.  CPU tensors run the
same definition in torch ops.
"""
from __future__ import annotations

import ctypes
import numbers

import torch
import torch.nn.functional as F

MAX_VIEWS = 8  # SEG_TTA_MAX_VIEWS


class SegTtaView(ctypes.Structure):
    """seg_tta_view (include/segamd.h)."""
    _fields_ = [("low", ctypes.c_void_p), ("ld", ctypes.c_long), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("flip", ctypes.c_int), ("weight", ctypes.c_float)]


class TTA:
    """The option object: scales in [0.5, 2], hflip adds each scale's mirrored view, weights = one positive number
    per scale (None: uniform).  ValueError for anything else, and for more than MAX_VIEWS views."""

    def __init__(self, scales=(1.0,), hflip: bool = True, weights=None):
        def number(v):
            return isinstance(v, numbers.Real) and not isinstance(v, bool)

        if isinstance(scales, numbers.Real):
            scales = (scales,)
        scales = tuple(scales)
        if not scales or not all(number(s) and 0.5 <= s <= 2.0 for s in scales):
            raise ValueError(f"TTA scales must be one or more numbers in [0.5, 2], got {scales!r}")
        if not isinstance(hflip, bool):
            raise ValueError(f"TTA hflip must be a bool, got {hflip!r}")
        if weights is None:
            weights = (1.0,) * len(scales)
        weights = tuple(weights)
        if len(weights) != len(scales) or not all(number(w) and 0.0 < w < float("inf") for w in weights):
            raise ValueError(f"TTA weights must be one positive number per scale, got {weights!r}")
        if len(set(float(s) for s in scales)) != len(scales):
            raise ValueError(f"TTA scales must differ from each other (a repeated scale is the same view twice), got "
                             f"{scales!r}")
        if len(scales) * (2 if hflip else 1) > MAX_VIEWS:
            raise ValueError(f"TTA allows at most {MAX_VIEWS} views, got {len(scales) * (2 if hflip else 1)}")
        self.scales = tuple(float(s) for s in scales)
        self.hflip = hflip
        self.weights = tuple(float(w) for w in weights)

    def views(self):
        """[(scale, flip, weight)] in view order, the weights summing to 1."""
        per = 2 if self.hflip else 1
        total = sum(self.weights) * per
        out = []
        for s, w in zip(self.scales, self.weights):
            out.append((s, False, w / total))
            if self.hflip:
                out.append((s, True, w / total))
        return out

    def __repr__(self):
        return f"TTA(scales={self.scales}, hflip={self.hflip}, weights={self.weights})"


def as_tta(tta):
    """None, a TTA, or the shorthand "hflip" -> None or a TTA."""
    if tta is None or isinstance(tta, TTA):
        return tta
    if isinstance(tta, str) and tta == "hflip":
        return TTA()
    raise ValueError(f"tta must be None, 'hflip' or a seg_amd.TTA, got {tta!r}")


def size_divisor(model) -> int:
    """What the engine asks of H and W: 32 for MobileNetV2UNet, 8 for UNet / LightUNet."""
    from .unet import LightUNet, MobileNetV2UNet, UNet
    model = getattr(model, "module", model)
    if isinstance(model, MobileNetV2UNet):
        return 32
    if isinstance(model, (UNet, LightUNet)):
        return 8
    raise TypeError(f"test-time augmentation needs a seg_amd model, got {type(model).__name__}")


def view_shapes(model, H: int, W: int, tta):
    """[(Hv, Wv, flip, weight)] of the views of an H x W input, in view order.  Two scales that round to the same
    size -- the same height or the same width -- are a ValueError."""
    tta = as_tta(tta)
    d = size_divisor(model)
    out, seen = [], {}
    for s, flip, w in tta.views():
        hw = (d * max(1, int(H * s / d + 0.5)), d * max(1, int(W * s / d + 0.5)))
        for axis, n in zip("HW", hw):  # one axis is enough: the other scale's view would be a distorted copy of it
            if seen.setdefault((axis, n), s) != s:
                raise ValueError(f"TTA scales {seen[(axis, n)]:g} and {s:g} both give views with {axis} = {n} of a "
                                 f"{H}x{W} input (sizes are multiples of {d})")
        out.append((hw[0], hw[1], flip, w))
    return out


def make_view(x: torch.Tensor, Hv: int, Wv: int, flip: bool) -> torch.Tensor:
    """The view tensor of a normalised NCHW batch: the bilinear (align_corners=False) resize to Hv x Wv, mirrored
    left-right when `flip`; x itself for the plain view of x's own size.  GPU tensors: seg_tta_view_nchw."""
    N, C, H, W = x.shape
    if (Hv, Wv) == (H, W) and not flip:
        return x
    if x.device.type == "cpu":
        v = x if (Hv, Wv) == (H, W) else F.interpolate(x, (Hv, Wv), mode="bilinear", align_corners=False)
        return torch.flip(v, (-1,)) if flip else v
    from ._lib import call
    x = x.contiguous()
    if x.dtype != torch.float32:
        raise ValueError(f"expected a float32 batch, got {x.dtype}")
    out = torch.empty((N, C, Hv, Wv), device=x.device, dtype=torch.float32)
    call("seg_tta_view_nchw", x.data_ptr(), N, C, H, W, out.data_ptr(), Hv, Wv, int(flip),
         torch.cuda.current_stream(x.device).cuda_stream)
    return out


def tta_probabilities(lows, flips, weights, out_hw) -> torch.Tensor:
    """The definition in torch ops: lows = the views' low-resolution logits as NCHW tensors [N, C, Hl_v, Wl_v],
    flips / weights per view (weights summing to 1) -> p [N, C, Ho, Wo] float32."""
    Ho, Wo = out_hw
    p = None
    for low, flip, w in zip(lows, flips, weights):
        z = low if tuple(low.shape[-2:]) == (Ho, Wo) else \
            F.interpolate(low, (Ho, Wo), mode="bilinear", align_corners=True)
        if flip:
            z = torch.flip(z, (-1,))
        term = torch.softmax(z.float(), dim=1) * w
        p = term if p is None else p + term
    return p


# ---------------------------------------------------------------------------------------------- CPU tensors
def _cpu_lows(model, x, shapes):
    from .export import torch_low_logits
    return [torch_low_logits(model, make_view(x, Hv, Wv, flip)) for Hv, Wv, flip, _ in shapes]


@torch.no_grad()
def torch_forward_tta(model, x, tta):
    shapes = view_shapes(model, x.shape[2], x.shape[3], tta)
    return tta_probabilities(_cpu_lows(model, x, shapes), [s[2] for s in shapes], [s[3] for s in shapes],
                             tuple(x.shape[2:]))


@torch.no_grad()
def torch_metrics_tta(model, x, target, confusion, tta, ignore_index=-100, weight=None, reduction="mean"):
    """forward_metrics_tta in torch ops (CPU tensors): F.nll_loss raises on an out-of-range label by itself."""
    from .metrics import add_confusion
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    p = torch_forward_tta(model, x, tta)
    loss = F.nll_loss(torch.log(p), target, weight=weight, ignore_index=ignore_index, reduction=reduction)
    add_confusion(confusion, p.argmax(1), target, ignore_index)
    return loss


# ---------------------------------------------------------------------------------------------- MI355X
def view_table(lows, flips, weights):
    """A host array of seg_tta_view over the views' NHWC float32 logits [N, Hl, Wl, ld] (kept alive by the caller)."""
    arr = (SegTtaView * len(lows))()
    for k, (low, flip, w) in enumerate(zip(lows, flips, weights)):
        if low.dtype != torch.float32 or low.dim() != 4 or not low.is_contiguous():
            raise ValueError("a view's logits must be a contiguous float32 [N, Hl, Wl, ld] tensor")
        arr[k].low, arr[k].ld = low.data_ptr(), low.shape[3]
        arr[k].H, arr[k].W = low.shape[1], low.shape[2]
        arr[k].flip, arr[k].weight = int(flip), float(w)
    return arr


def _gpu_lows(model, x, shapes):
    from .engine import run_low_logits
    return [run_low_logits(model, make_view(x, Hv, Wv, flip)) for Hv, Wv, flip, _ in shapes]


def _run(model, x, tta, target, confusion, ignore_index, weight, reduction, want_prob):
    from ._lib import call, query
    from .engine import _check_input, get_program, loss_options
    _check_input(x)
    x = x.contiguous()
    N, _, H, W = x.shape
    shapes = view_shapes(model, H, W, tta)
    prog = get_program(model, N, H, W)
    Ho, Wo = prog.out_hw
    C = prog.logits.C
    dev = x.device
    if C > 32:
        raise ValueError(f"test-time augmentation's validation kernel takes up to 32 classes, the model has {C}")
    t = None  # forward_tta: no labels -- the kernel writes the probabilities alone
    if target is not None:
        t = target.contiguous()
        if t.dtype != torch.int64 or tuple(t.shape) != (N, Ho, Wo) or t.device != dev:
            raise ValueError(f"target must be int64 [{N},{Ho},{Wo}] on {dev}, got {tuple(t.shape)} {t.dtype} "
                             f"on {t.device}")
        if (confusion.dtype != torch.int64 or tuple(confusion.shape) != (C, C) or confusion.device != dev
                or not confusion.is_contiguous()):
            raise ValueError(f"confusion must be a contiguous int64 [{C},{C}] tensor on {dev}, got "
                             f"{tuple(confusion.shape)} {confusion.dtype} on {confusion.device}")
    weight, _, reduction, _ = loss_options(weight, 0.0, reduction, C, dev)
    lows = _gpu_lows(model, x, shapes)
    views = view_table(lows, [s[2] for s in shapes], [s[3] for s in shapes])
    work = torch.empty(query("seg_tta_workspace_floats", N * Ho * Wo), dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.float32, device=dev)
    prob = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=dev) if want_prob else None
    with torch.cuda.device(dev):
        call("seg_tta_upsample_eval", ctypes.addressof(views), len(lows), N, C, t.data_ptr() if t is not None else None,
             Ho, Wo, ignore_index, weight.data_ptr() if weight is not None else None,
             0 if reduction == "mean" else 1, work.data_ptr(), stats.data_ptr(),
             confusion.data_ptr() if t is not None else None, prob.data_ptr() if prob is not None else None,
             torch.cuda.current_stream(dev).cuda_stream)
    return stats, prob


@torch.no_grad()
def run_forward_tta(model, x, tta):
    return _run(model, x, tta, None, None, -100, None, "mean", True)[1]


@torch.no_grad()
def run_metrics_tta(model, x, target, confusion, tta, ignore_index=-100, weight=None, reduction="mean"):
    """The ensemble's validation step on the MI355X; the out-of-range label count is published as run_metrics
    publishes it (engine.bad_label_count)."""
    from .engine import _publish_stats
    stats, _ = _run(model, x, tta, target, confusion, ignore_index, weight, reduction, False)
    return _publish_stats(model, stats)
