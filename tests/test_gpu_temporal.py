"""GPU: seg_temporal_argmax_nearest (csrc/infer.hip) called directly on synthetic low-res logits, against
the float64 restatement (tests/temporal_ref.py) computed from the same float32 logits.

  * the state after every frame of a four-frame sequence, alpha in {1, 0.5, 0.25}: |s - s_ref| <= 1e-5
    (the per-frame fp32 error of the blend, expf and a <= 255-term sum on probabilities in [0, 1] is of
    order 1e-6; the recurrence is a convex combination, so it does not accumulate; x10 margin);
  * labels == the restatement's wherever its top-2 margin exceeds 1e-4 and its maximum is further than
    1e-5 from the threshold (test_temporal_ref.py: at most 1 % of the pixels are not), and everywhere
    == classify() of the kernel's own state; mask == INTER_NEAREST of the labels, exactly;
  * pad lanes (+1e30 in the logits, NaN in the state) never matter; the fresh word; a non-finite frame.
Cases: tests/temporal_cases.py (both model shapes, the three frame sizes, C in {1, 3, 10, 19}, a state
row wider than the logits', N = 2, a confidence threshold).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_cases as cases  # noqa: E402
import temporal_ref as ref  # noqa: E402

from seg_amd._lib import call  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


class Buffers:
    """Device buffers of one case: the state and its pad lanes start as NaN, the word as fresh."""

    def __init__(self, case):
        self.case = case
        H, W, Hm, Wm = cases.SHAPES[case.shape]
        Hf, Wf = case.frame_hw
        self.low = torch.empty((case.N, H, W, case.ld), device=DEV, dtype=torch.float32)
        self.state = torch.full((case.N * Hm * Wm, case.state_ld), float("nan"), device=DEV, dtype=torch.float32)
        self.fresh = torch.ones(1, device=DEV, dtype=torch.int32)
        self.labels = torch.full((case.N, Hm, Wm), 255, device=DEV, dtype=torch.uint8)
        self.mask = torch.full((case.N, Hf, Wf), 255, device=DEV, dtype=torch.uint8)

    def step(self, low, alpha):
        """One call on the float32 logits `low`; returns (state [N, C, Hm, Wm], labels, mask) as numpy."""
        c = self.case
        H, W, Hm, Wm = cases.SHAPES[c.shape]
        self.low.copy_(torch.from_numpy(low))
        call("seg_temporal_argmax_nearest", self.low.data_ptr(), c.ld, c.N, H, W, c.C, Hm, Wm, self.state.data_ptr(),
             c.state_ld, self.fresh.data_ptr(), alpha, c.min_conf, c.fallback, self.labels.data_ptr(),
             self.mask.data_ptr(), c.frame_hw[0], c.frame_hw[1], torch.cuda.current_stream().cuda_stream)
        s = self.state.cpu().numpy().reshape(c.N, Hm, Wm, c.state_ld)[..., :c.C].transpose(0, 3, 1, 2)
        return s, self.labels.cpu().numpy(), self.mask.cpu().numpy()


def check_exact_parts(case, state, labels, mask):
    """argmax, threshold and nearest are exact operations: the labels follow from the kernel's own state
    and the mask from its labels."""
    for n in range(case.N):
        own = ref.classify(state[n], np.float32(case.min_conf), case.fallback)
        np.testing.assert_array_equal(labels[n], own)
        np.testing.assert_array_equal(mask[n], ref.to_frame(labels[n], case.frame_hw))


@pytest.mark.parametrize("alpha", cases.ALPHAS)
@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_sequence_matches_reference(case, alpha, record):
    buf = Buffers(case)
    worst, excluded = 0.0, 0.0
    for t, want in enumerate(cases.answers(case, alpha)):
        state, labels, mask = buf.step(cases.logits(case, t), alpha)
        assert int(buf.fresh.item()) == 0  # cleared by the first call, and stays so
        assert np.isfinite(state).all()    # the NaN the state started with is gone after a fresh frame
        worst = max(worst, float(np.abs(state - want.state).max()))
        excluded = max(excluded, float((~want.decided).mean()))
        np.testing.assert_array_equal(labels[want.decided], want.labels[want.decided])
        check_exact_parts(case, state, labels, mask)
        if t == 0:  # a fresh state: s = p, whatever alpha
            assert np.abs(state - cases.answers(case, 1.0)[0].state).max() <= TOL
        if case.min_conf > 0:
            assert 0.2 <= (labels == case.fallback).mean() <= 0.9
    record(case=case.name, alpha=alpha, worst_abs_err=worst, bound=TOL, worst_excluded_fraction=excluded)
    print(f"{case.name} alpha {alpha}: worst |s - s_ref| {worst:.3e} (bound {TOL:g}), excluded {excluded:.4f}")
    assert excluded <= 0.01
    assert worst <= TOL, worst


def test_pad_lanes_are_left_alone():
    """The state's quads past the logits' (lds > ld) are never written, and the pad lanes of the written
    quads hold 0; neither is read into a result (the sequence test compares those)."""
    case = cases.BY_NAME["wide-state-c10"]
    buf = Buffers(case)
    buf.step(cases.logits(case, 0), 0.5)
    buf.step(cases.logits(case, 1), 0.5)
    rows = buf.state.cpu().numpy()
    assert np.all(rows[:, case.C:case.ld] == 0) and np.isnan(rows[:, case.ld:]).all()


def test_alpha_one_forgets_the_state():
    """alpha == 1 takes p itself: bitwise the state a fresh call gives, whatever the state held."""
    case = cases.BY_NAME["banded-c10"]
    a, b = Buffers(case), Buffers(case)
    a.step(cases.logits(case, 0), 1.0)
    sa, la, ma = a.step(cases.logits(case, 1), 1.0)
    sb, lb, mb = b.step(cases.logits(case, 1), 0.25)  # fresh
    assert np.array_equal(sa, sb) and np.array_equal(la, lb) and np.array_equal(ma, mb)


@pytest.mark.parametrize("name", ["banded-c10", "odd-model-c19"])
def test_non_finite_frame(name):
    """Frame 2 holds one NaN and one +Inf logit: exactly the model pixels with one of them among their
    four taps keep their state bitwise, the others update; frame 3 matches the reference everywhere;
    the same frame on a fresh state leaves the uniform 1/C there."""
    case, alpha = cases.BY_NAME[name], 0.5
    H, W, Hm, Wm = cases.SHAPES[case.shape]
    lows = [cases.logits(case, t) for t in range(3)]
    lows[1] = lows[1].copy()
    lows[1][0, H // 3, W // 4, 2] = np.nan
    lows[1][0, H - 1, W // 2, 0] = np.inf
    want = cases.run(case, alpha, lows)
    hit = ~np.isfinite(cases.model_logits(case, lows[1])).all(axis=1)[0]
    # the taps of a model pixel are the low-res pixels around its source position: two small patches
    assert 2 <= hit.sum() <= hit.size // 4 and hit[Hm - 1].any() and not hit[Hm - 1].all()
    buf = Buffers(case)
    s1, _, _ = buf.step(lows[0], alpha)
    s2, l2, m2 = buf.step(lows[1], alpha)
    assert np.array_equal(s2[0][:, hit], s1[0][:, hit])
    assert np.all(np.abs(s2[0] - s1[0]).max(axis=0)[~hit] > 0)
    assert np.abs(s2 - want[1].state).max() <= TOL
    check_exact_parts(case, s2, l2, m2)
    s3, l3, m3 = buf.step(lows[2], alpha)
    assert np.isfinite(s3).all() and np.abs(s3 - want[2].state).max() <= TOL
    check_exact_parts(case, s3, l3, m3)
    np.testing.assert_array_equal(l3[want[2].decided], want[2].labels[want[2].decided])
    # on a fresh (NaN-filled) state
    fresh = Buffers(case)
    f, lf, mf = fresh.step(lows[1], alpha)
    assert np.all(f[0][:, hit] == np.float32(1) / np.float32(case.C))
    assert np.abs(f - cases.run(case, alpha, lows[1:2])[0].state).max() <= TOL
    assert np.all(lf[0][hit] == 0)  # the first of C equal maxima
    check_exact_parts(case, f, lf, mf)


def test_fresh_word_restarts_the_average():
    """Setting the word again (what Predictor.reset() does) gives bitwise a new buffer's first frame."""
    case = cases.BY_NAME["small-frame-c3"]
    a, b = Buffers(case), Buffers(case)
    a.step(cases.logits(case, 0), 0.25)
    a.step(cases.logits(case, 1), 0.25)
    a.fresh.fill_(1)
    sa, la, ma = a.step(cases.logits(case, 2), 0.25)
    sb, lb, mb = b.step(cases.logits(case, 2), 0.25)
    assert np.array_equal(sa, sb) and np.array_equal(la, lb) and np.array_equal(ma, mb)
    assert int(a.fresh.item()) == 0
