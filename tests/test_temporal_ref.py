"""CPU: the temporal-smoothing restatement (tests/temporal_ref.py) has the properties the GPU tests lean on,
the C entry validates its arguments before any launch, and Predictor rejects bad options before it looks
for a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_cases as cases  # noqa: E402
import temporal_ref as ref  # noqa: E402

from seg_amd import UNet, _lib  # noqa: E402
from seg_amd.build import build  # noqa: E402
from seg_amd.infer import Predictor, temporal_options  # noqa: E402

NAME = "seg_temporal_argmax_nearest"


def fields(C, H, W, seed, frames=4):
    g = np.random.Generator(np.random.PCG64(seed))
    return [g.normal(0, 2.5, (C, H, W)) for _ in range(frames)]


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.25])
def test_state_rows_sum_to_one(alpha):
    s = None
    for z in fields(10, 9, 13, seed=1):
        s = ref.step(s, z, alpha)
        assert np.abs(s.sum(axis=0) - 1).max() < 1e-12
        assert s.min() >= 0


def test_alpha_one_is_the_per_frame_argmax():
    s = None
    for z in fields(7, 9, 13, seed=2):
        s = ref.step(s, z, 1.0)
        np.testing.assert_allclose(s, ref.softmax(z), rtol=0, atol=1e-15)
        np.testing.assert_array_equal(ref.classify(s), np.argmax(z, axis=0))


def test_constant_input_is_a_fixed_point():
    z = fields(5, 6, 7, seed=3, frames=1)[0]
    s = ref.step(None, z, 0.25)
    for _ in range(5):
        s = ref.step(s, z, 0.25)
    np.testing.assert_allclose(s, ref.softmax(z), rtol=0, atol=1e-15)


def test_non_finite_frame_keeps_the_state():
    z0, z1, z2 = fields(4, 6, 7, seed=4, frames=3)
    s0 = ref.step(None, z0, 0.5)
    bad = z1.copy()
    bad[2, 1, 3] = np.nan
    bad[0, 4, 5] = np.inf
    bad[1, 2, 2] = -np.inf
    s1 = ref.step(s0, bad, 0.5)
    hit = np.zeros((6, 7), bool)
    hit[1, 3] = hit[4, 5] = hit[2, 2] = True
    np.testing.assert_array_equal(s1[:, hit], s0[:, hit])
    np.testing.assert_array_equal(s1[:, ~hit], ref.step(s0, z1, 0.5)[:, ~hit])
    assert np.isfinite(s1).all()
    # the next frame updates every pixel as usual
    s2 = ref.step(s1, z2, 0.5)
    np.testing.assert_array_equal(s2, s1 + 0.5 * (ref.softmax(z2) - s1))
    # a whole NaN frame changes nothing; on a fresh state the hit pixels are uniform
    np.testing.assert_array_equal(ref.step(s0, np.full_like(z1, np.nan), 0.5), s0)
    f = ref.step(None, bad, 0.5)
    assert np.all(f[:, hit] == 0.25) and np.array_equal(f[:, ~hit], ref.softmax(z1)[:, ~hit])


def test_classify_threshold_and_first_maximum():
    s = np.array([[0.5, 0.2, 0.4], [0.5, 0.2, 0.35], [0.0, 0.6, 0.25]])[:, None, :]
    np.testing.assert_array_equal(ref.classify(s), [[0, 2, 0]])           # the first of two equal maxima
    np.testing.assert_array_equal(ref.classify(s, 0.45, 1), [[0, 2, 1]])  # 0.4 < 0.45 -> fallback
    np.testing.assert_array_equal(ref.classify(s, 0.5, 1), [[0, 2, 1]])   # max == threshold stays
    np.testing.assert_array_equal(ref.to_frame(ref.classify(s), (2, 6)), [[0, 0, 2, 2, 0, 0]] * 2)


def test_upsample_is_the_align_corners_bilinear():
    torch = pytest.importorskip("torch")
    low = fields(3, 5, 7, seed=5, frames=1)[0]
    want = torch.nn.functional.interpolate(torch.from_numpy(low)[None], size=(9, 13), mode="bilinear",
                                           align_corners=True)[0].numpy()
    # float32 source coordinates (as the kernels form them) against torch's float64 ones
    np.testing.assert_allclose(ref.upsample(low, 9, 13), want, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(ref.upsample(low, 5, 7), low)
    bad = low.copy()
    bad[1, 2, 3] = np.inf
    up = ref.upsample(bad, 9, 13)
    assert not np.isfinite(up[1, 4, 6]) and np.isfinite(up[0]).all() and np.isfinite(up[1, 0, 0])


# ---------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_kernel_cases_are_decided(case):
    """A condition on the inputs, met by the restatement alone: at most 1 % of the model pixels of any
    frame have a top-2 margin <= 1e-4 or lie within 1e-5 of the threshold (the GPU test compares labels
    on the others); the threshold cases put a good part of the pixels on either side of 0.3 and under
    0.1 % within 1e-5 of it; the logits stay within |z| <= amp."""
    for t in range(cases.FRAMES):
        low = cases.logits(case, t)
        assert low.dtype == np.float32 and np.abs(low[..., :case.C]).max() <= case.amp * (1 + 1e-6)
        assert np.all(low[..., case.C:] == np.float32(cases.PAD_LOGIT))
    for alpha in cases.ALPHAS:
        for a in cases.answers(case, alpha):
            assert (~a.decided).mean() <= 0.01, (alpha, (~a.decided).mean())
            if case.min_conf > 0:
                conf = a.state.max(axis=1)
                below = (conf < case.min_conf).mean()
                assert 0.2 <= below <= 0.8, (alpha, below)
                assert (np.abs(conf - case.min_conf) <= 1e-5).mean() < 1e-3
                assert np.array_equal(a.labels == case.fallback, (conf < case.min_conf) | (a.state.argmax(1) == case.fallback))


# ---------------------------------------------------------------- the C entry
@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.lib()


def test_prototype_is_declared():
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == 19


def test_invalid_arguments_are_rejected_before_any_launch(lib):
    """hipErrorInvalidValue (1) for every invalid case, each alone among otherwise valid arguments: host
    addresses stand in for state / fresh / labels, which a rejected call never touches (this test
    needs no GPU); low and mask stay null as in test_abi.py."""
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(low=None, ld=12, N=1, H=16, W=32, C=10, Hm=32, Wm=64, state=ptr, lds=12, fresh=ptr, alpha=0.5,
              min_conf=0.3, fallback=9, labels=ptr, mask=None, Hf=90, Wf=160, stream=None)
    cases = [dict(ld=10), dict(ld=8), dict(lds=14), dict(lds=8), dict(C=0), dict(C=256, ld=256, lds=256),
             dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.5), dict(alpha=float("nan")), dict(min_conf=-0.1),
             dict(min_conf=1.1), dict(min_conf=float("nan")), dict(fallback=-1), dict(fallback=10), dict(state=None),
             dict(fresh=None), dict(labels=None)]
    for bad in cases:
        assert getattr(lib, NAME)(*{**ok, **bad}.values()) == 1, bad
    # and with every pointer null, as the other entries are probed
    for bad in cases:
        args = {**ok, "state": None, "fresh": None, "labels": None, **bad}
        assert getattr(lib, NAME)(*args.values()) == 1, bad


# ---------------------------------------------------------------- Predictor's options
def test_options_helper():
    assert temporal_options(None) is None
    assert temporal_options(None, 0.0, 3) is None
    assert temporal_options(0.5) == (0.5, 0.0, 0)
    assert temporal_options(1, 0.25, 2, classes=3) == (1.0, 0.25, 2)
    assert temporal_options(None, 0.3, 9, classes=10) == (1.0, 0.3, 9)   # alpha 1.0 with the threshold alone
    assert temporal_options(np.float32(0.25), np.float64(0.5), np.int64(1)) == (0.25, 0.5, 1)
    for bad in (dict(temporal=0.0), dict(temporal=-0.1), dict(temporal=1.01), dict(temporal=float("nan")),
                dict(temporal="0.5"), dict(temporal=True), dict(min_confidence=-1e-3), dict(min_confidence=1.5),
                dict(min_confidence=None), dict(min_confidence=float("nan")), dict(fallback_class=-1),
                dict(fallback_class=1.0), dict(fallback_class=10, classes=10),
                dict(temporal=0.5, fallback_class=10, classes=10)):
        with pytest.raises(ValueError):
            temporal_options(**{"temporal": None, **bad})


def test_predictor_rejects_bad_options_before_it_needs_a_gpu():
    model = UNet(10, 16)  # on the CPU: valid options reach the device check, bad ones never do
    for kw in (dict(temporal=0.0), dict(temporal=2.0), dict(min_confidence=1.5), dict(fallback_class=-1)):
        with pytest.raises(ValueError):
            Predictor(model, frame_hw=(22, 40), target_size=(64, 32), **kw)
    with pytest.raises(RuntimeError):
        Predictor(model, frame_hw=(22, 40), target_size=(64, 32), temporal=0.5, min_confidence=0.3)
