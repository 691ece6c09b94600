"""Inputs and float64 answers of the kernel-level temporal-smoothing tests, shared by the CPU test that
checks the inputs (test_temporal_ref.py) and the GPU test that uses them (test_gpu_temporal.py).

A case is a short sequence of synthetic low-res logits: smooth random fields (a coarse random grid,
bilinearly enlarged, plus a little noise) scaled to |z| <= amp, a part of which carries over from frame to
frame.  The answers are computed once per (case, alpha) and are read-only.
"""
from typing import NamedTuple

import numpy as np

import temporal_ref as ref

SHAPES = {"32x64": (16, 32, 32, 64), "9x13": (5, 7, 9, 13)}  # low H, W -> model Hm, Wm
ALPHAS = (1.0, 0.5, 0.25)
FRAMES = 4
PAD_LOGIT = 1e30  # what the logits' pad lanes hold


class Case(NamedTuple):
    name: str
    shape: str
    frame_hw: tuple
    C: int
    N: int = 1
    lds: int = 0          # 0: C rounded up to 4, like ld
    min_conf: float = 0.0
    fallback: int = 0
    amp: float = 6.0
    seed: int = 0

    @property
    def ld(self):
        return (self.C + 3) // 4 * 4

    @property
    def state_ld(self):
        return self.lds or self.ld


CASES = [
    Case("banded-c10", "32x64", (90, 160), 10, seed=1),
    Case("odd-width-c19", "32x64", (61, 166), 19, seed=2),
    Case("small-frame-c3", "32x64", (22, 40), 3, seed=3),
    Case("banded-c1", "32x64", (90, 160), 1, seed=4),
    Case("odd-model-c19", "9x13", (90, 160), 19, seed=5),
    Case("odd-model-odd-width-c10", "9x13", (61, 166), 10, seed=6),
    Case("odd-model-c1", "9x13", (22, 40), 1, seed=7),
    Case("odd-model-odd-width-c3", "9x13", (61, 166), 3, seed=8),
    Case("wide-state-c10", "32x64", (22, 40), 10, lds=16, seed=9),
    Case("batch2-c10", "9x13", (90, 160), 10, N=2, seed=10),
    Case("batch2-c19", "32x64", (61, 166), 19, N=2, seed=11),
    Case("threshold-c10", "32x64", (90, 160), 10, min_conf=0.3, fallback=9, amp=5.0, seed=12),
    Case("threshold-small-frame-c10", "32x64", (22, 40), 10, min_conf=0.3, fallback=9, amp=5.0, seed=13),
]
BY_NAME = {c.name: c for c in CASES}


def _field(g, C, H, W):
    coarse = g.normal(0, 1, (C, 3, 4))
    return ref.upsample(coarse, H, W) + 0.15 * g.normal(0, 1, (C, H, W))


def logits(case, t):
    """float32 [N, H, W, ld] low-res logits of frame t, pad lanes at PAD_LOGIT."""
    H, W, _, _ = SHAPES[case.shape]
    out = np.full((case.N, H, W, case.ld), PAD_LOGIT, np.float32)
    for n in range(case.N):
        base = _field(np.random.Generator(np.random.PCG64([case.seed, n, 1000])), case.C, H, W)
        x = 0.6 * base + 0.4 * _field(np.random.Generator(np.random.PCG64([case.seed, n, t])), case.C, H, W)
        out[n, :, :, :case.C] = (case.amp * x / np.abs(x).max()).transpose(1, 2, 0)
    return out


def model_logits(case, low):
    """float64 [N, C, Hm, Wm]: the upsample of the float32 low-res logits."""
    _, _, Hm, Wm = SHAPES[case.shape]
    return np.stack([ref.upsample(low[n, :, :, :case.C].transpose(2, 0, 1), Hm, Wm) for n in range(case.N)])


class Answer(NamedTuple):
    state: np.ndarray    # float64 [N, C, Hm, Wm]
    labels: np.ndarray   # uint8 [N, Hm, Wm]
    mask: np.ndarray     # uint8 [N, Hf, Wf]
    decided: np.ndarray  # bool [N, Hm, Wm]: ref.decided


def answer(case, state):
    labels = np.stack([ref.classify(s, case.min_conf, case.fallback) for s in state])
    out = Answer(state, labels, np.stack([ref.to_frame(c, case.frame_hw) for c in labels]),
                 np.stack([ref.decided(s, case.min_conf) for s in state]))
    for a in out:
        a.setflags(write=False)
    return out


def run(case, alpha, lows, state=None):
    """[Answer per frame] of the float32 low-res logits `lows`, from `state` ([N, C, Hm, Wm] or None: fresh)."""
    out = []
    for low in lows:
        z = model_logits(case, low)
        state = np.stack([ref.step(None if state is None else state[n], z[n], alpha) for n in range(case.N)])
        out.append(answer(case, state))
    return out


_ANSWERS = {}


def answers(case, alpha):
    """The case's own FRAMES frames from a fresh state, computed once."""
    key = (case.name, alpha)
    if key not in _ANSWERS:
        _ANSWERS[key] = run(case, alpha, [logits(case, t) for t in range(FRAMES)])
    return _ANSWERS[key]
