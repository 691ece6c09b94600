"""GPU replacement for the per-frame path of the reference's inference.py.

The reference loop (inference.py:150-170) does, per video frame:
    img_tensor, _ = preprocess_image(frame)            # :28-46  cv2.resize -> RGB -> ToTensor -> Normalize
    road_predictions = model(img_tensor)               # :162-163 eval forward under no_grad
    _, cls = torch.max(road_predictions, dim=1)        # :64     (inside overlay_predictions)
    cls = cv2.resize(cls.astype(uint8), (W, H), INTER_NEAREST)   # :68-70
and then overlay_predictions' OpenCV post-processing (inference.py:72-146), which
seg_amd/overlay.py runs on the GPU (`Predictor(..., overlay=True)`), and the display.

`Predictor` runs all of that on the MI355X as four stages over static buffers,
captured once into a HIP graph (torch.cuda.CUDAGraph drives hipGraph on ROCm):
    seg_preprocess_bgr      uint8 BGR frame -> the model's NHWC4 input rows
    Run.forward_folded      eval forward, BatchNorm folded into every conv
                            (Program.fold: one seg_bn_fold_batch + one seg_pack_batch)
    seg_argmax_nearest      final align_corners=True upsample + argmax + nearest
                            resize to the frame -> uint8 class mask
                            (seg_temporal_argmax_nearest with `temporal=` / `min_confidence=`:
                            the argmax of the class probabilities averaged over the frames;
                            seg_tta_argmax_nearest with `tta=`: the argmax of the probabilities averaged
                            over the flipped / rescaled views, behind seg_preprocess_bgr_views and one
                            folded forward per view size)

`preprocess_image` mirrors inference.py's function of the same name (same
argument meaning and return values) for callers that still want the tensor.
"""
from __future__ import annotations

import ctypes
import numbers

import numpy as np
import torch

from ._lib import call
from . import engine
from .engine import Run, get_program

MEAN = (0.485, 0.456, 0.406)   # inference.py:35
STD = (0.229, 0.224, 0.225)    # inference.py:36


def _frame_tensor(frame, device) -> torch.Tensor:
    if isinstance(frame, np.ndarray):
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError(f"expected a uint8 HxWx3 BGR frame, got {frame.dtype} {frame.shape}")
        return torch.from_numpy(np.ascontiguousarray(frame)).to(device, non_blocking=False)
    if not torch.is_tensor(frame) or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError("expected a uint8 HxWx3 BGR frame (numpy array or tensor)")
    return frame.to(device).contiguous()


def preprocess_image(image, target_size=(256, 128), device="cuda"):
    """inference.py:28-46 on the GPU: returns (img_tensor [1,3,H,W] float32 on
    `device`, the resized RGB uint8 image is not materialised -> None)."""
    W, H = target_size  # cv2 dsize order (width, height)
    f = _frame_tensor(image, device)
    Hf, Wf = f.shape[0], f.shape[1]
    rows = torch.empty((H * W, 4), device=f.device, dtype=torch.float32)
    s = torch.cuda.current_stream(f.device).cuda_stream
    call("seg_preprocess_bgr", f.data_ptr(), 1, Hf, Wf, f.stride(0), rows.data_ptr(), 4, H, W, *MEAN, *STD, s)
    img = rows[:, :3].reshape(1, H, W, 3).permute(0, 3, 1, 2).contiguous()
    return img, None


def temporal_options(temporal, min_confidence=0.0, fallback_class=0, classes=None):
    """Validate Predictor's smoothing options.  Returns None when the feature is off (temporal None and
    min_confidence 0), else (alpha, min_confidence, fallback_class) as seg_temporal_argmax_nearest takes
    them; alpha is 1.0 (no smoothing) when only min_confidence is given.  `classes`: the model's class
    count, when known, bounds fallback_class."""
    def number(v):
        return isinstance(v, numbers.Real) and not isinstance(v, bool)

    if temporal is not None and not (number(temporal) and 0.0 < temporal <= 1.0):
        raise ValueError(f"Predictor temporal must be None or the newest frame's weight in (0, 1], got {temporal!r}")
    if not (number(min_confidence) and 0.0 <= min_confidence <= 1.0):
        raise ValueError(f"Predictor min_confidence must lie in [0, 1], got {min_confidence!r}")
    if not isinstance(fallback_class, numbers.Integral) or isinstance(fallback_class, bool) or fallback_class < 0:
        raise ValueError(f"Predictor fallback_class must be a class index >= 0, got {fallback_class!r}")
    if classes is not None and fallback_class >= classes:
        raise ValueError(f"Predictor fallback_class {fallback_class} is not one of the model's {classes} classes")
    if temporal is None and min_confidence == 0:
        return None
    return (1.0 if temporal is None else float(temporal)), float(min_confidence), int(fallback_class)


class Predictor:
    """Frame -> class mask for a MobileNetV2UNet / UNet in eval mode.

    predictor = Predictor(model, frame_hw=(720, 1280))   # model already on cuda
    mask = predictor(frame)          # uint8 [720, 1280] class ids on the GPU
    logits = predictor.logits()      # [1, C, 128, 256] of the last frame (tests)

    math="f16" runs every folded conv on fp16 operands (BASELINE configs[3]).
    Weights are folded at construction; call `refresh()` after changing the
    model's parameters or running statistics (e.g. load_state_dict).

    overlay=True (or an `Overlay` instance) appends overlay_predictions' post-processing
    (seg_amd/overlay.py) to the launch sequence and the graph:
    result, detected_objects = predictor.annotate(frame); `__call__` still returns the mask.

    temporal=alpha (0 < alpha <= 1) classifies video: the mask is the argmax of an exponential moving
    average of the per-pixel class probabilities, s += alpha (softmax(logits) - s), kept at model
    resolution across frames (seg_temporal_argmax_nearest in place of seg_argmax_nearest, inside the
    graph too); min_confidence > 0 paints pixels whose largest averaged probability is below it with
    fallback_class.  Either option switches the path on (alpha 1.0 when only min_confidence is given).
    `reset()` starts a new average (scene cut, seek); `probabilities()` / `confidence()` read it.

    tta (a seg_amd.TTA, or "hflip") classifies the frame from a test-time-augmentation ensemble (seg_amd/tta.py has
    the definition): every view is formed straight from the frame at its own size (seg_preprocess_bgr_views: nothing
    is resized twice), the plain and the mirrored view of one size run as ONE batch-2 folded forward (inference is
    launch-bound at batch 1), and seg_tta_argmax_nearest replaces seg_argmax_nearest, inside the graph too.
    min_confidence / fallback_class act on the ensemble's p as they act on the temporal average, and
    `probabilities()` / `confidence()` read p; a view whose logits are non-finite at a pixel is left out there.
    tta_batch=False runs every view as a batch-1 forward of its own instead -- what math="f16" always does: its
    fused inverted-residual launches are batch-1 routes, so tta_batch=True is a ValueError there.  tta together
    with temporal is a ValueError.

    threshold (a probability in (0, 1); None: the argmax path, unchanged) classifies a one-channel model: the mask is
    1 where the upsampled logit is > log(threshold / (1 - threshold)) -- strictly, so a tie or a NaN logit is
    background -- else 0 (seg_threshold_nearest in place of seg_argmax_nearest, inside the graph too).  The mask feeds
    the overlay unchanged: its road = (cls == 1) is the model's foreground.  A model with more channels, or threshold
    together with temporal, min_confidence or tta, is a ValueError.
    """

    def __init__(self, model, frame_hw=(720, 1280), target_size=(256, 128), graph: bool = True, math: str = "f32",
                 overlay=False, temporal: float | None = None, min_confidence: float = 0.0, fallback_class: int = 0,
                 tta=None, tta_batch: bool | None = None, threshold: float | None = None):
        temporal_options(temporal, min_confidence, fallback_class)  # bad values: ValueError before anything else
        self.zthr = None  # None: every line of the argmax path as it always was
        if threshold is not None:
            from .losses import logit_threshold
            if not isinstance(threshold, numbers.Real) or isinstance(threshold, bool):
                raise ValueError(f"Predictor threshold must be None or a probability in (0, 1), got {threshold!r}")
            self.zthr = logit_threshold(threshold)
            if temporal is not None or min_confidence != 0 or tta is not None:
                raise ValueError("Predictor threshold cannot be combined with temporal, min_confidence or tta: "
                                 "smoothing or ensembling a one-logit model is not implemented")
        from .tta import as_tta
        self.tta = as_tta(tta)
        if self.tta is not None and temporal is not None:
            raise ValueError("Predictor tta and temporal cannot be combined: averaging the ensemble's probabilities "
                             "over the frames is not implemented")
        if tta_batch is not None and not isinstance(tta_batch, bool):
            raise ValueError(f"Predictor tta_batch must be None or a bool, got {tta_batch!r}")
        if self.tta is not None and tta_batch and math == "f16":
            raise ValueError("Predictor tta_batch=True is not available with math='f16': its fused folded routes "
                             "(seg_mbconv_f16, seg_pw2_f16) run at batch 1 only")
        p = next(model.parameters())
        if not p.is_cuda:
            raise RuntimeError("Predictor runs on the MI355X HIP path only; move the model to 'cuda' first")
        self.model = model.eval()
        self.device = p.device
        self.Hf, self.Wf = frame_hw
        self.W, self.H = target_size
        # math: conv arithmetic of the folded forward -- "f32" (the reference's), "f16"
        # (BASELINE configs[3]: fp16 operands, fp32 accumulation) or "bf16"
        if math not in ("f32", "f16", "bf16"):
            raise ValueError(f"Predictor math must be 'f32', 'f16' or 'bf16', got {math!r}")
        self.frame = torch.zeros((self.Hf, self.Wf, 3), device=self.device, dtype=torch.uint8)
        self.mask = torch.empty((self.Hf, self.Wf), device=self.device, dtype=torch.uint8)
        self.run = None
        if self.tta is None:
            self.prog = get_program(model, 1, self.H, self.W, math)
            self.run = Run(self.prog, self.frame, training=False)
        else:
            self._tta_setup(model, math, math != "f16" if tta_batch is None else tta_batch)
            # the output grid and the class count are the scale-1 program's: a view group's own when one has that
            # size (whatever its batch), else a program built for them alone (no buffers: it never runs)
            same = [g[1] for g in self._tta_groups if (g[1].image.H, g[1].image.W) == (self.H, self.W)]
            self.prog = same[0] if same else get_program(model, 1, self.H, self.W, math)
        self.classes = self.prog.logits.C
        if self.zthr is not None and self.classes != 1:
            raise ValueError(f"Predictor threshold needs a model with one output channel, this one has {self.classes}")
        self.temporal =temporal_options(temporal, min_confidence, fallback_class, self.classes)
        if self.tta is not None and self.temporal is None:
            self.temporal = (1.0, 0.0, 0)  # the state, labels and readers of the smoothing path; no threshold
        if self.temporal is not None:
            Ho, Wo = self.prog.out_hw
            lds = (self.classes + 3) // 4 * 4
            # the average [Ho*Wo][lds], the word that starts a new one (not with tta), the classes at model resolution
            self._state = torch.zeros((Ho * Wo, lds), device=self.device, dtype=torch.float32)
            if self.tta is None:
                self._fresh = torch.ones(1, device=self.device, dtype=torch.int32)
            self._labels = torch.zeros((Ho, Wo), device=self.device, dtype=torch.uint8)
        self.graph = None
        self.refresh()
        self.stem_pre = self.prog.stem_pre() if (engine.STEM_PRE and math == "f16" and self.tta is None) else None
        self.overlay = None
        if overlay is not False and overlay is not None:
            from .overlay import Overlay
            self.overlay = Overlay(frame_hw, device=self.device) if overlay is True else overlay
            if not isinstance(self.overlay, Overlay) or (self.overlay.Hf, self.overlay.Wf) != (self.Hf, self.Wf):
                raise ValueError(f"overlay must be True or an Overlay for {self.Hf}x{self.Wf} frames")
        if graph:
            self._capture()
            if self.temporal is not None and self.tta is None:
                self.reset()  # the warm-up launch of the capture averaged the empty frame buffer

    def refresh(self):
        """Re-fold BatchNorm into the conv weights (after weights/statistics change)."""
        with torch.no_grad():
            s = torch.cuda.current_stream(self.device).cuda_stream
            if self.tta is None:
                self.prog.fold(s)
            else:
                for prog in {id(g[1]): g[1] for g in self._tta_groups}.values():  # every view size's program
                    prog.fold(s)

    def _tta_setup(self, model, math, batch):
        """One folded-forward group per view size (batch: its plain and mirrored view as one batch) or per view:
        (Run, Program, copies, flip_mask); the views' order and weights are TTA.views()."""
        from .tta import view_shapes
        shapes = view_shapes(model, self.H, self.W, self.tta)
        self._tta_weights = [w for _, _, _, w in shapes]
        self._tta_groups = []
        k = 0
        while k < len(shapes):
            Hv, Wv, flip, _ = shapes[k]
            n = 2 if batch and k + 1 < len(shapes) and shapes[k + 1][:2] == (Hv, Wv) else 1
            mask = sum(int(shapes[k + i][2]) << i for i in range(n))
            prog = get_program(model, n, Hv, Wv, math)
            self._tta_groups.append((Run(prog, self.frame, training=False), prog, n, mask))
            k += n

    def _launch_tta(self, s):
        from .tta import SegTtaView
        views = (SegTtaView * len(self._tta_weights))()
        k = 0
        for rt, prog, n, mask in self._tta_groups:
            rt.stream = s
            img, lo = prog.image, prog.logits
            call("seg_preprocess_bgr_views", self.frame.data_ptr(), self.Hf, self.Wf, self.frame.stride(0),
                 rt.ptr(img), img.ld, img.H, img.W, n, mask, *MEAN, *STD, s)
            rt.forward_folded()
            for i in range(n):
                v = views[k]
                v.low, v.ld, v.H, v.W = rt.ptr(lo) + 4 * i * lo.H * lo.W * lo.ld, lo.ld, lo.H, lo.W
                v.flip, v.weight = (mask >> i) & 1, self._tta_weights[k]
                k += 1
        Ho, Wo = self.prog.out_hw
        _, min_conf, fallback = self.temporal
        call("seg_tta_argmax_nearest", ctypes.addressof(views), len(views), 1, self.classes, Ho, Wo,
             self._state.data_ptr(), self._state.shape[1], min_conf, fallback, self._labels.data_ptr(),
             self.mask.data_ptr(), self.Hf, self.Wf, s)
        if self.overlay is not None:
            self.overlay.launch(self.frame, self.mask, s)

    def _launch(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        if self.tta is not None:
            return self._launch_tta(s)
        rt, prog = self.run, self.prog
        rt.stream = s
        img = prog.image
        if self.stem_pre is not None:  # preprocess formed on load by the stem conv (seg_stem_pre_f16)
            op, o = self.stem_pre, self.stem_pre.out
            call("seg_stem_pre_f16", self.frame.data_ptr(), self.Hf, self.Wf, self.frame.stride(0), self.H, self.W,
                 *MEAN, *STD, op.fk_pack.data_ptr(), op.ldk_f, op.fb.data_ptr(), op.act, op.cout, rt.ptr(o), o.ld, s)
            rt.forward_folded(start=1)
        else:
            call("seg_preprocess_bgr", self.frame.data_ptr(), 1, self.Hf, self.Wf, self.frame.stride(0), rt.ptr(img),
                 img.ld, self.H, self.W, *MEAN, *STD, s)
            rt.forward_folded()
        lo = prog.logits
        Ho, Wo = prog.out_hw
        if self.zthr is not None:  # a one-logit model: the mask {0, 1} is z > zthr, the overlay's road its foreground
            call("seg_threshold_nearest", rt.ptr(lo), lo.ld, 1, lo.H, lo.W, Ho, Wo, self.zthr, self.mask.data_ptr(),
                 self.Hf, self.Wf, s)
        elif self.temporal is None:
            call("seg_argmax_nearest", rt.ptr(lo), lo.ld, 1, lo.H, lo.W, lo.C, Ho, Wo, self.mask.data_ptr(), self.Hf,
                 self.Wf, s)
        else:
            alpha, min_conf, fallback = self.temporal
            call("seg_temporal_argmax_nearest", rt.ptr(lo), lo.ld, 1, lo.H, lo.W, lo.C, Ho, Wo,
                 self._state.data_ptr(), self._state.shape[1], self._fresh.data_ptr(), alpha, min_conf, fallback,
                 self._labels.data_ptr(), self.mask.data_ptr(), self.Hf, self.Wf, s)
        if self.overlay is not None:
            self.overlay.launch(self.frame, self.mask, s)

    def _capture(self):
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            self._launch()  # warm-up outside the capture (module load, first-launch setup)
        torch.cuda.current_stream(self.device).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._launch()
        self.graph = g

    def set_frame(self, frame):
        """Copy a frame into the static input buffer (host numpy -> H2D, or device tensor)."""
        if isinstance(frame, np.ndarray):
            if frame.shape != (self.Hf, self.Wf, 3) or frame.dtype != np.uint8:
                raise ValueError(f"expected uint8 frame of shape {(self.Hf, self.Wf, 3)}, got {frame.dtype} "
                                 f"{frame.shape}")
            self.frame.copy_(torch.from_numpy(np.ascontiguousarray(frame)), non_blocking=False)
        else:
            if tuple(frame.shape) != (self.Hf, self.Wf, 3) or frame.dtype != torch.uint8:
                raise ValueError(f"expected uint8 frame of shape {(self.Hf, self.Wf, 3)}")
            self.frame.copy_(frame)

    def step(self):
        """Run the captured graph (or the eager launch sequence) on the current frame."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._launch()
        return self.mask

    def __call__(self, frame=None):
        if frame is not None:
            self.set_frame(frame)
        return self.step()

    def annotate(self, frame=None):
        """(result, detected_objects) of inference.py's overlay_predictions for the frame: the uint8
        [Hf, Wf, 3] blended frame on the GPU (a static buffer) and {'cars': n}."""
        if self.overlay is None:
            raise RuntimeError("annotate() needs Predictor(..., overlay=True)")
        self(frame)
        return self.overlay.result, self.overlay.detected_objects()

    def reset(self):
        """Start a new average with the next frame (a scene cut, a seek): sets the device word the update
        kernel reads, in stream order; the captured graph stays as it is.  refresh() does not reset."""
        if self.temporal is None or self.tta is not None:
            raise RuntimeError("reset() needs Predictor(..., temporal=alpha) or min_confidence > 0, without tta")
        self._fresh.fill_(1)

    def probabilities(self) -> torch.Tensor:
        """[1, C, H, W] float32 view of the averaged class probabilities s_t after the last frame (with tta: of the
        ensemble's p)."""
        if self.temporal is None:
            raise RuntimeError("probabilities() needs Predictor(..., temporal=alpha), min_confidence > 0 or tta")
        Ho, Wo = self.prog.out_hw
        return self._state.view(1, Ho, Wo, -1)[..., :self.classes].permute(0, 3, 1, 2)

    def confidence(self) -> torch.Tensor:
        """[H, W] float32: the largest averaged class probability of every model pixel."""
        return self.probabilities()[0].amax(dim=0)

    def logits(self) -> torch.Tensor:
        """[1, C, H, W] logits of the last frame (the model's return value, src/unet.py:49)."""
        if self.tta is not None:
            raise RuntimeError("logits() has no meaning for a tta ensemble of several views; read probabilities()")
        lo = self.prog.logits
        Ho, Wo = self.prog.out_hw
        out = torch.empty((1, lo.C, Ho, Wo), device=self.device, dtype=torch.float32)
        call("seg_upsample_to_nchw", self.run.ptr(lo), lo.ld, 1, lo.H, lo.W, lo.C, out.data_ptr(), Ho, Wo, 1,
             torch.cuda.current_stream(self.device).cuda_stream)
        return out
