"""Pure-numpy float64 restatement of the test-time-augmentation ensemble (seg_amd/tta.py,
seg_tta_upsample_eval, seg_tta_argmax_nearest), for the tests.  Built on temporal_ref.py's pieces.

Per view v (low-resolution logits L_v [C, Hl_v, Wl_v], a flip flag, a weight; the weights are normalised to
sum 1) and output pixel (y, x) of the Ho x Wo grid:  z_v = the align_corners=True bilinear sample of L_v at
(y, x_v), x_v = Wo - 1 - x for a mirrored view -- the source coordinate and tap index formed in float32, as the
kernels form them -- p = sum_v w_v softmax(z_v);  class = the first maximum of p.  Arrays are channel-first.
"""
import numpy as np

from temporal_ref import classify, margin, softmax, to_frame, upsample  # noqa: F401  (re-exported)
from temporal_ref import decided as _decided


def normalised(weights):
    """The kernels' weights: the float32 inputs divided by their sum (in float64)."""
    w = np.asarray(np.asarray(weights, np.float32), np.float64)
    return w / w.sum()


def view_logits(low, flip, out_hw):
    """z_v [C, Ho, Wo] in float64: the upsample of the float32 logits, mirrored by indexing the upsampled array."""
    z = upsample(low, out_hw[0], out_hw[1])
    return z[:, :, ::-1] if flip else z


def probabilities(lows, flips, weights, out_hw):
    """p [C, Ho, Wo] of validation's rule: every view counts; a non-finite logit makes the pixel's p NaN."""
    w = normalised(weights)
    with np.errstate(invalid="ignore"):
        return sum(wk * softmax(view_logits(low, f, out_hw)) for low, f, wk in zip(lows, flips, w))


def probabilities_guarded(lows, flips, weights, out_hw):
    """p of the Predictor's rule: a view with a non-finite z_v at a pixel is left out there and the remaining
    weights are renormalised; none left: 1/C."""
    w = normalised(weights)
    C = lows[0].shape[0]
    num = np.zeros((C,) + tuple(out_hw))
    den = np.zeros(tuple(out_hw))
    for low, f, wk in zip(lows, flips, w):
        z = view_logits(low, f, out_hw)
        ok = np.isfinite(z).all(axis=0)
        num += np.where(ok[None], wk * softmax(np.where(ok[None], z, 0.0)), 0.0)
        den += np.where(ok, wk, 0.0)
    return np.where(den[None] > 0, num / np.where(den > 0, den, 1.0)[None], 1.0 / C)


def decided(p, min_confidence=0.0):
    """The project's thresholds: top-2 margin > 1e-4, maximum further than 1e-5 from min_confidence."""
    return _decided(p, min_confidence)


def nll(p, labels, ignore_index=-100, class_weight=None, reduction="mean"):
    """nn.NLLLoss(class_weight, ignore_index, reduction)(log p, labels) over a batch: p [N, C, H, W], labels
    [N, H, W]; returns (loss, D, #valid)."""
    N, C = p.shape[:2]
    w = np.ones(C) if class_weight is None else np.asarray(class_weight, np.float64)
    valid = labels != ignore_index
    y = np.where(valid, labels, 0)
    py = np.take_along_axis(p, y[:, None], axis=1)[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(valid, -w[y] * np.log(py), 0.0)
    d = np.where(valid, w[y], 0.0).sum() if reduction == "mean" else 1.0
    return terms.sum() / d, d, int(valid.sum())


def confusion(classes, labels, C, ignore_index=-100):
    """int64 [C, C]: confusion[label, class] over the valid pixels."""
    valid = labels != ignore_index
    idx = labels[valid].astype(np.int64) * C + classes[valid].astype(np.int64)
    return np.bincount(idx, minlength=C * C).reshape(C, C)
