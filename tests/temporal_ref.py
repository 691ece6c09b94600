"""Pure-numpy float64 restatement of the temporal smoothing of class probabilities
(seg_temporal_argmax_nearest, `Predictor(..., temporal=alpha)`), for the tests.

Per model pixel and frame t:  p_t = softmax_c(z_t);  s_t = p_t on a fresh state, else
s_{t-1} + alpha (p_t - s_{t-1});  class = the first maximum of s_t, or the fallback class where that
maximum is below min_confidence;  mask = cv2 INTER_NEAREST of the classes to the frame.  A pixel with a
non-finite logit keeps s_{t-1} (the uniform 1/C on a fresh state).  Arrays are channel-first: [C, H, W].
"""
import numpy as np

from oracle.cvresize import resize_nearest


def upsample(low, Hm, Wm):
    """align_corners=True bilinear upsample of low-res logits [C, H, W] to [C, Hm, Wm] in float64: the
    model's z_t from the kernel's input.  The source coordinate and the tap index are formed in float32,
    as the kernels form them, so both blend the same taps; the weights and the blend are float64.  A
    non-finite tap makes the pixel non-finite whatever its weight (0 * inf = nan)."""
    low = np.asarray(low, np.float64)
    _, H, W = low.shape

    def taps(n_out, n_in):
        scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
        src = scale * np.arange(n_out, dtype=np.float32)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = np.clip(src.astype(np.float64) - i0, 0.0, 1.0)
        return i0, i1, 1.0 - l1, l1

    y0, y1, h0, h1 = taps(Hm, H)
    x0, x1, w0, w1 = taps(Wm, W)
    with np.errstate(invalid="ignore"):
        top = low[:, y0][:, :, x0] * w0 + low[:, y0][:, :, x1] * w1
        bot = low[:, y1][:, :, x0] * w0 + low[:, y1][:, :, x1] * w1
        return top * h0[None, :, None] + bot * h1[None, :, None]


def softmax(z):
    """softmax over axis 0 of [C, ...] in float64, max-subtracted."""
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - z.max(axis=0, keepdims=True))
        return e / e.sum(axis=0, keepdims=True)


def step(s_prev, logits, alpha):
    """s_t [C, H, W] from s_{t-1} (None: a fresh state) and the frame's logits z_t [C, H, W]."""
    z = np.asarray(logits, np.float64)
    C = z.shape[0]
    ok = np.isfinite(z).all(axis=0)
    p = softmax(np.where(ok[None], z, 0.0))
    if s_prev is None:
        return np.where(ok[None], p, 1.0 / C)
    s_prev = np.asarray(s_prev, np.float64)
    return np.where(ok[None], s_prev + alpha * (p - s_prev), s_prev)


def classify(s, min_confidence=0.0, fallback_class=0):
    """uint8 [H, W]: the first maximum over the channels of s, the fallback below min_confidence."""
    cls = np.argmax(s, axis=0).astype(np.uint8)
    cls[s.max(axis=0) < min_confidence] = fallback_class
    return cls


def to_frame(cls, frame_hw):
    Hf, Wf = frame_hw
    return resize_nearest(cls, (Wf, Hf))


def margin(s):
    """top-1 minus top-2 of s over the channels (inf for a single channel)."""
    if s.shape[0] == 1:
        return np.full(s.shape[1:], np.inf)
    top = np.sort(s, axis=0)[-2:]
    return top[1] - top[0]


def decided(s, min_confidence=0.0):
    """Pixels whose class no rounding of s can change: the top-2 margin exceeds 1e-4 and the maximum is
    further than 1e-5 from the threshold."""
    ok = margin(s) > 1e-4
    if min_confidence > 0:
        ok &= np.abs(s.max(axis=0) - min_confidence) > 1e-5
    return ok
