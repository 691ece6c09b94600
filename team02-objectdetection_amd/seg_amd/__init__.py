"""seg_amd -- MI355X-native hot path for SEAME-pt/Team02-ObjectDetection's
segmentation models (MobileNetV2UNet / UNet / LightUNet).

Public surface (drop-in for the reference's src/unet.py and src/train.py):
    MobileNetV2UNet, UNet, LightUNet, double_conv, inconv, down, up, outconv
    train_model, train_one_epoch
    validate, summarize                   (validation loss, per-class IoU, mIoU: one fused pass per batch)
    class_weights                         (nn.CrossEntropyLoss(weight=...) from pixel counts or a confusion matrix)
    SegLoss                               (cross-entropy with a focal exponent plus soft Dice, fused like CE)
    OhemCELoss                            (cross-entropy with online hard example mining, fused like CE)
    BinarySegLoss, binary_summary         (one-logit models: sigmoid BCE / focal / Dice, fused like CE; validation
                                           thresholds the logit and reports precision, recall and F1)
    DistillLoss                           (knowledge distillation: CE plus the tempered KL to a teacher's logits,
                                           both models' final upsamples fused into the loss kernels)
    Adam                                  (main.py:100's optimizer, one-launch HIP step)
    AdamW, decay_groups                   (torch.optim.AdamW as a one-launch HIP step; decayed / undecayed groups)
    SGD                                   (torch.optim.SGD -- momentum, Nesterov, L2 weight decay -- as a
                                           one-launch HIP step)
    PolyLR                                (the poly learning-rate decay with a linear warm-up; train_model(...,
                                           scheduler=) steps it after every optimizer step)
    grad_norm, clip_grad_norm_            (global L2 gradient norm and clipping on the device)
    EMA                                   (exponential moving average of the weights: one launch per step,
                                           exchanged in place with the live weights for evaluation)
    TTA, view_shapes                      (test-time augmentation: flip / multi-scale ensembles for validate,
                                           Predictor, model.forward_tta / forward_metrics_tta; one fused kernel)
    traceable                             (pure-torch CPU twin for convert.py's ONNX export)
    freeze, unfreeze, frozen_modules      (fine-tuning: frozen backbone / frozen BatchNorm statistics)
    Predictor, preprocess_image           (inference.py's per-frame path)
    Overlay, overlay_predictions, COLOR_MAP
                                          (inference.py's overlay post-processing)
    CombinedLaneDataset, DistributedWeightedSampler, reference_sample_weights
                                          (main.py's data path, rank-aware)
All compute runs in libsegamd.so (HIP, gfx950); see include/segamd.h.
"""
from .unet import MobileNetV2UNet, UNet, LightUNet, double_conv, inconv, down, up, outconv  # noqa: F401
from .train import train_model, train_one_epoch, validate  # noqa: F401
from .metrics import binary_summary, class_weights, summarize  # noqa: F401
from .losses import BinarySegLoss, DistillLoss, OhemCELoss, SegLoss  # noqa: F401
from .detinit import deterministic_init, synthetic_batch  # noqa: F401
from .data import CombinedLaneDataset, DistributedWeightedSampler, reference_sample_weights  # noqa: F401
from .infer import Predictor, preprocess_image  # noqa: F401
from .overlay import Overlay, overlay_predictions, COLOR_MAP  # noqa: F401
from .optim import SGD, Adam, AdamW, clip_grad_norm_, decay_groups, grad_norm  # noqa: F401
from .schedule import PolyLR  # noqa: F401
from .ema import EMA  # noqa: F401
from .export import traceable  # noqa: F401
from .tta import TTA, view_shapes  # noqa: F401
from .freeze import freeze, unfreeze, frozen_modules  # noqa: F401

__all__ = ["MobileNetV2UNet", "UNet", "LightUNet", "double_conv", "inconv", "down", "up", "outconv",
           "train_model", "train_one_epoch", "validate", "summarize", "class_weights", "SegLoss", "OhemCELoss",
           "DistillLoss", "BinarySegLoss", "binary_summary",
           "deterministic_init",
           "synthetic_batch",
           "CombinedLaneDataset", "DistributedWeightedSampler", "reference_sample_weights",
           "Predictor", "preprocess_image", "Overlay", "overlay_predictions", "COLOR_MAP",
           "Adam", "AdamW", "SGD", "PolyLR", "clip_grad_norm_", "decay_groups", "grad_norm", "EMA", "TTA",
           "view_shapes",
           "traceable", "freeze", "unfreeze", "frozen_modules"]
