"""GPU: `Predictor(..., temporal=alpha, min_confidence=, fallback_class=)` -- the class mask of the
exponential moving average of the per-pixel class probabilities over a frame sequence, against the
float64 restatement (tests/temporal_ref.py) run on the predictor's own per-frame logits().

The sequence: the frame() recipe of test_gpu_infer.py with seeds 3, 4, 5, 6, the last two mirrored left to
right (a scene change).  Bounds: the state within 1e-5 (see test_gpu_temporal.py); the mask equal to the
restatement's outside the pixels whose top-2 margin is <= 1e-4 (at most 1 % of them), and exactly the
argmax + INTER_NEAREST of the predictor's own probabilities().
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref  # noqa: E402
import temporal_ref as ref  # noqa: E402

from oracle import cvresize  # noqa: E402
from seg_amd import Overlay, UNet, deterministic_init  # noqa: E402
from seg_amd.infer import Predictor  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE = (64, 32)  # cv2 order: the model sees 32 x 64
TOL = 1e-5


def frame(h, w, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.linspace(0, 6, h), np.linspace(0, 9, w), indexing="ij")
    base = 127.5 + 100 * np.sin(yy)[..., None] * np.cos(xx[..., None] + np.arange(3))
    return np.clip(base + g.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def sequence(fh, fw):
    fs = [frame(fh, fw, s) for s in (3, 4, 5, 6)]
    return fs[:2] + [np.ascontiguousarray(f[:, ::-1]) for f in fs[2:]]


@pytest.fixture(scope="module")
def model():
    return deterministic_init(UNet(10, 16), seed=11, random_running_stats=True).to(DEV)


def predictor(model, fhw, **kw):
    kw.setdefault("graph", True)
    return Predictor(model, frame_hw=fhw, target_size=SIZE, **kw)


def np_state(pred):
    return pred.probabilities()[0].cpu().numpy()


@pytest.mark.parametrize("alpha", [0.5, 0.25])
@pytest.mark.parametrize("fhw", [(90, 160), (22, 40), (61, 166)])
def test_sequence_matches_reference(model, fhw, alpha, record):
    pred = predictor(model, fhw, temporal=alpha)
    plain = predictor(model, fhw)
    s, worst, excluded, differs = None, 0.0, 0.0, []
    for f in sequence(*fhw):
        mask = pred(f).cpu().numpy()
        z = pred.logits()[0].double().cpu().numpy()
        s = ref.step(s, z, alpha)
        got = np_state(pred)
        assert got.shape == (10, 32, 64) and got.dtype == np.float32
        worst = max(worst, float(np.abs(got - s).max()))
        decided = ref.decided(s)
        excluded = max(excluded, float((~decided).mean()))
        keep = ref.to_frame(decided, fhw)
        assert np.array_equal(mask[keep], ref.to_frame(ref.classify(s), fhw)[keep])
        np.testing.assert_array_equal(mask, cvresize.class_mask(pred.probabilities().cpu().numpy(), fhw))
        np.testing.assert_array_equal(pred.confidence().cpu().numpy(), got.max(axis=0))
        differs.append(float((mask != plain(f).cpu().numpy()).mean()))
    record(frame_hw=fhw, alpha=alpha, worst_abs_err=worst, bound=TOL, worst_excluded_fraction=excluded,
           differs_from_per_frame=differs)
    print(f"{fhw} alpha {alpha}: worst |s - s_ref| {worst:.3e}, excluded {excluded:.4f}, differs from the "
          f"per-frame mask {differs}")
    assert excluded <= 0.01
    assert worst <= TOL, worst
    assert differs[0] < 0.005  # one frame: the average is the frame (but for an fp32 tie of two probabilities)
    assert differs[2] > 0.05   # the smoothing is really on


def test_graph_equals_eager_with_reset(model):
    fhw = (61, 166)
    g = predictor(model, fhw, temporal=0.25, min_confidence=0.3, fallback_class=9)
    e = predictor(model, fhw, temporal=0.25, min_confidence=0.3, fallback_class=9, graph=False)
    assert g.graph is not None and e.graph is None
    for i, f in enumerate(sequence(*fhw)):
        if i == 2:
            g.reset()
            e.reset()
        assert torch.equal(g(f), e(f))
        assert torch.equal(g.probabilities(), e.probabilities())
        assert torch.equal(g.logits(), e.logits())


def test_reset_and_fixed_point(model):
    fhw = (22, 40)
    fs = sequence(*fhw)
    pred = predictor(model, fhw, temporal=0.5)
    for f in fs[:2]:
        pred(f)
    pred.reset()
    pred.refresh()  # does not reset (and does not undo one)
    mask = pred(fs[2]).clone()
    new = predictor(model, fhw, temporal=0.5)
    assert torch.equal(new(fs[2]), mask) and torch.equal(new.probabilities(), pred.probabilities())
    # the frame after a reset is the frame's own softmax; replays on a constant frame stay there
    p = ref.softmax(pred.logits()[0].double().cpu().numpy())
    assert np.abs(np_state(pred) - p).max() <= TOL
    first = np_state(pred).copy()
    for _ in range(6):
        pred.step()
    assert np.abs(np_state(pred) - first).max() <= 1e-6
    assert torch.equal(pred.mask, mask)
    # without a reset the next frame is averaged in: not the new predictor's answer
    pred(fs[3])
    new.reset()
    new(fs[3])
    assert not torch.equal(new.probabilities(), pred.probabilities())


def test_alpha_one_is_the_plain_mask(model):
    fhw = (90, 160)
    pred = predictor(model, fhw, temporal=1.0)
    plain = predictor(model, fhw)
    for f in sequence(*fhw)[1:3]:
        mask = pred(f).cpu().numpy()
        want = plain(f).cpu().numpy()
        z = plain.logits()[0].double().cpu().numpy()
        top2 = np.sort(z, axis=0)[-2:]
        confident = ref.to_frame(top2[1] - top2[0], fhw) > 1e-3 * np.abs(z).max()
        assert confident.mean() > 0.9
        assert np.array_equal(mask[confident], want[confident])
        assert np.abs(np_state(pred) - ref.softmax(z)).max() <= TOL


def test_min_confidence_alone(model):
    """min_confidence without temporal: alpha 1.0, every frame on its own, uncertain pixels to the fallback."""
    fhw = (90, 160)
    pred = predictor(model, fhw, min_confidence=0.3, fallback_class=9)
    assert pred.temporal == (1.0, 0.3, 9)
    for f in sequence(*fhw)[:2]:
        mask = pred(f).cpu().numpy()
        s = np_state(pred)
        assert np.abs(s - ref.softmax(pred.logits()[0].double().cpu().numpy())).max() <= TOL
        below = s.max(axis=0) < np.float32(0.3)
        assert 0.2 < below.mean() < 0.8, below.mean()
        np.testing.assert_array_equal(mask, ref.to_frame(ref.classify(s, np.float32(0.3), 9), fhw))
        assert np.all(ref.to_frame(below, fhw) <= (mask == 9))


def test_two_predictors_on_two_streams(model):
    fhw = (61, 166)
    seqs = [sequence(*fhw), sequence(*fhw)[::-1]]
    solo = []
    for fs in seqs:
        p = predictor(model, fhw, temporal=0.5)
        out = []
        for f in fs:
            out.append((p(f).clone(), p.probabilities().clone()))
        solo.append(out)
    preds = [predictor(model, fhw, temporal=0.5) for _ in seqs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    frames = [[torch.from_numpy(f).to(DEV) for f in fs] for fs in seqs]
    torch.cuda.synchronize()
    got = [[], []]
    for t in range(4):
        for k, (p, st) in enumerate(zip(preds, streams)):
            with torch.cuda.stream(st):
                p(frames[k][t])
                got[k].append((p.mask.clone(), p.probabilities().clone()))
    torch.cuda.synchronize()
    for k in range(2):
        for (m, s), (m0, s0) in zip(got[k], solo[k]):
            assert torch.equal(m, m0) and torch.equal(s, s0)
    assert not torch.equal(got[0][3][1], got[1][3][1])


def test_overlay_follows_the_smoothed_mask(model):
    fhw = (22, 40)
    kw = dict(min_area=3, max_boxes=8)
    pred = predictor(model, fhw, overlay=Overlay(fhw, **kw), temporal=0.5)
    plain = predictor(model, fhw)
    for i, f in enumerate(sequence(*fhw)[1:3]):
        res, det = pred.annotate(f)
        mask = pred.mask.cpu().numpy()
        want_res, want_cleaned, want_boxes, want_det = overlay_ref.overlay(f, mask, **kw)
        assert np.array_equal(res.cpu().numpy(), want_res)
        assert np.array_equal(pred.overlay.cleaned.cpu().numpy(), want_cleaned)
        assert pred.overlay.boxes() == want_boxes and det == want_det
        np.testing.assert_array_equal(mask, cvresize.class_mask(pred.probabilities().cpu().numpy(), fhw))
        if i == 1:
            assert not np.array_equal(mask, plain(f).cpu().numpy())


def test_low_precision_math(model):
    fhw = (90, 160)
    pred = predictor(model, fhw, temporal=0.5, math="f16")
    s = None
    for f in sequence(*fhw)[1:3]:
        pred(f)
        s = ref.step(s, pred.logits()[0].double().cpu().numpy(), 0.5)
        assert pred.probabilities().dtype == torch.float32
        assert np.abs(np_state(pred) - s).max() <= TOL


def test_defaults_are_the_plain_path(model):
    fhw = (90, 160)
    pred = predictor(model, fhw)
    assert pred.temporal is None
    f = sequence(*fhw)[0]
    mask = pred(f).cpu().numpy()
    np.testing.assert_array_equal(mask, cvresize.class_mask(pred.logits().cpu().numpy(), fhw))
    # the same bits as the entry the plain path has always called
    lo, (Ho, Wo) = pred.prog.logits, pred.prog.out_hw
    from seg_amd._lib import call
    direct = torch.full(fhw, 255, device=DEV, dtype=torch.uint8)
    call("seg_argmax_nearest", pred.run.ptr(lo), lo.ld, 1, lo.H, lo.W, lo.C, Ho, Wo, direct.data_ptr(), fhw[0],
         fhw[1], torch.cuda.current_stream().cuda_stream)
    assert torch.equal(direct, pred.mask)
    for fn in (pred.probabilities, pred.confidence, pred.reset):
        with pytest.raises(RuntimeError):
            fn()
