"""Inputs and float64 answers of the kernel-level test-time-augmentation tests, shared by the CPU test that
checks the inputs (test_tta.py) and the GPU test that uses them (test_gpu_tta.py).

A case is a set of views of N images: per view float32 low-resolution logits [N, Hl, Wl, ld], iid N(0, 3^2) in
the C real lanes and PAD_LOGIT in the pad lanes, a flip flag and a weight; int64 labels on the output grid with
about a tenth of them ignored; optionally class weights and a confidence threshold.  The shapes are the smallest
that reach each hazard: the x2 model's grid (8x16 -> 16x32), other scales' (6x12, 10x20, 12x24 -> 16x32: one
interpolation at a non-integer ratio), UNet's (16x32 -> 16x32: no upsample), an odd output grid whose mirror
axis falls on a pixel (15x31), C in {1, 3, 10, 19, 32} (every register variant of both kernels and the
Predictor's any-C variant), rows wider than round4(C), 1 / 2 / 6 / 8 views, unequal weights, and one case of
2 x 512 x 520 = 532480 pixels: the smallest that takes both kernels' capped grids (2048 blocks of 256 and 8192
of 64 pixels: 524288) round their grid-stride loops twice.  Answers are computed once per case and read-only.
"""
from typing import NamedTuple

import numpy as np

import tta_ref as ref

PAD_LOGIT = 1e30
SIGMA = 3.0


class Case(NamedTuple):
    name: str
    out_hw: tuple
    views: tuple          # ((Hl, Wl, flip, weight), ...)
    C: int
    seed: int
    N: int = 2
    extra_ld: int = 0     # lanes beyond round4(C)
    ignore_index: int = -100
    class_weight: bool = False
    reduction: str = "mean"
    min_conf: float = 0.0
    fallback: int = 0
    frame_hw: tuple = (45, 80)

    @property
    def ld(self):
        return (self.C + 3) // 4 * 4 + self.extra_ld


def pair(H, W, w=1.0):
    return ((H, W, False, w), (H, W, True, w))


CASES = [
    Case("x2-hflip-c10", (16, 32), pair(8, 16), 10, seed=1),
    Case("x2-single-c10", (16, 32), ((8, 16, False, 1.0),), 10, seed=2),
    Case("x2-mirror-only-c3", (16, 32), ((8, 16, True, 2.5),), 3, seed=3, frame_hw=(37, 61)),
    Case("scales6-weights-c19", (16, 32), pair(6, 12, 0.5) + pair(8, 16, 2.0) + pair(10, 20, 1.0), 19, seed=4,
         ignore_index=255, class_weight=True),
    Case("scales8-c3", (16, 32), pair(6, 12) + pair(8, 16) + pair(10, 20) + pair(12, 24), 3, seed=5,
         reduction="sum"),
    Case("unet-hflip-c32", (16, 32), pair(16, 32), 32, seed=6, class_weight=True),
    Case("unet-scales-c1", (16, 32), pair(16, 32, 3.0) + pair(24, 48, 1.0), 1, seed=7),
    Case("odd-grid-c3", (15, 31), pair(8, 16) + pair(5, 11, 0.25), 3, seed=8, frame_hw=(37, 61)),
    Case("odd-grid-c19", (15, 31), pair(8, 16), 19, seed=9, ignore_index=255),
    Case("wide-rows-c10", (16, 32), pair(8, 16) + pair(10, 20, 0.5), 10, seed=10, extra_ld=4),
    Case("wide-rows-c32", (15, 31), pair(8, 16), 32, seed=11, extra_ld=8, reduction="sum", class_weight=True),
    Case("threshold-c10", (16, 32), pair(8, 16), 10, seed=12, min_conf=0.35, fallback=9),
    Case("c20-any", (16, 32), pair(8, 16) + ((10, 20, False, 0.7),), 20, seed=13),
    # the register variants the classes above leave out (2, 4, 6 and 7 channel quads)
    Case("x2-hflip-c7", (16, 32), pair(8, 16), 7, seed=15),
    Case("x2-hflip-c16", (15, 31), pair(8, 16), 16, seed=16, N=1),
    Case("x2-hflip-c24", (16, 32), pair(8, 16), 24, seed=17, N=1),
    Case("x2-hflip-c28", (15, 31), pair(8, 16), 28, seed=18, N=1, class_weight=True),
    Case("grid-stride-c3", (512, 520), pair(256, 260), 3, seed=14, frame_hw=(64, 68)),
]
BY_NAME = {c.name: c for c in CASES}


def _rng(case, *key):
    return np.random.Generator(np.random.PCG64([case.seed, *key]))


def lows(case):
    """[float32 [N, Hl, Wl, ld] per view]: N(0, SIGMA^2) logits, pad lanes at PAD_LOGIT."""
    out = []
    for k, (H, W, _, _) in enumerate(case.views):
        a = np.full((case.N, H, W, case.ld), PAD_LOGIT, np.float32)
        # a flip pair shares nothing: the mirrored view's logits are a forward of their own
        a[..., :case.C] = _rng(case, 1, k).normal(0.0, SIGMA, (case.N, H, W, case.C))
        out.append(a)
    return out


def labels(case):
    """int64 [N, Ho, Wo]: uniform classes, about a tenth ignore_index."""
    g = _rng(case, 2)
    y = g.integers(0, case.C, (case.N,) + case.out_hw).astype(np.int64)
    y[g.random(y.shape) < 0.1] = case.ignore_index
    return y


def class_weight(case):
    """float32 [C] in [0.5, 2), or None."""
    return _rng(case, 3).uniform(0.5, 2.0, case.C).astype(np.float32) if case.class_weight else None


def flips(case):
    return [v[2] for v in case.views]


def weights(case):
    return [v[3] for v in case.views]


def channel_first(case, low, n):
    return low[n, :, :, :case.C].transpose(2, 0, 1)


class Answer(NamedTuple):
    p: np.ndarray          # float64 [N, C, Ho, Wo]
    classes: np.ndarray    # uint8 [N, Ho, Wo]: first maximum of p (validation)
    labels: np.ndarray     # uint8 [N, Ho, Wo]: ... with the fallback below min_conf (Predictor)
    decided: np.ndarray    # bool [N, Ho, Wo]
    loss: float
    D: float
    valid: int


def compute(case, view_lows, guarded=False):
    fn = ref.probabilities_guarded if guarded else ref.probabilities
    p = np.stack([fn([channel_first(case, lo, n) for lo in view_lows], flips(case), weights(case), case.out_hw)
                  for n in range(case.N)])
    with np.errstate(invalid="ignore"):
        classes = np.stack([ref.classify(s) for s in p])
        lab = np.stack([ref.classify(s, case.min_conf, case.fallback) for s in p])
        dec = np.stack([ref.decided(s, case.min_conf) for s in p])
    loss, d, valid = ref.nll(p, labels(case), case.ignore_index, class_weight(case), case.reduction)
    out = Answer(p, classes, lab, dec, float(loss), float(d), valid)
    for a in out[:4]:
        a.setflags(write=False)
    return out


_ANSWERS = {}


def answer(case):
    if case.name not in _ANSWERS:
        _ANSWERS[case.name] = compute(case, lows(case))
    return _ANSWERS[case.name]
