"""GPU: the test-time-augmentation kernels called directly (csrc/tta.hip, csrc/infer.hip) on the synthetic cases of
tests/tta_cases.py, against the float64 restatement (tests/tta_ref.py) computed from the same float32 inputs.

  * p: |p - p_ref| <= 1e-5 -- test_gpu_temporal.py's bound for one fp32 softmax of an interpolated logit row; p is
    a convex combination of at most 8 of them, so the bound carries over;
  * classes / labels: the reference's wherever it is decided (test_tta.py: at most 1 % of a case's pixels are
    not), and everywhere classify() of the kernel's own p; mask == INTER_NEAREST of the labels, exactly;
  * confusion == the bincount of the kernel's own classes, exactly, its total == out4's valid count;
  * loss within test_gpu_eval_metrics.py's tolerance for seg_cew_upsample_eval (the same kind of sum, of the same
    length): 1e-5 relative + 1e-7;
  * two runs bitwise equal; pad lanes never matter and are not written; the non-finite rules; the view and
    preprocess kernels.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_cases as cases  # noqa: E402
import tta_ref as ref  # noqa: E402

from seg_amd._lib import call, query  # noqa: E402
from seg_amd.tta import view_table  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_views(case, view_lows):
    lows = [torch.from_numpy(lo).to(DEV) for lo in view_lows]
    return lows, view_table(lows, cases.flips(case), cases.weights(case))


def run_eval(case, view_lows, want_prob=True, labels=None):
    """seg_tta_upsample_eval -> (out4, confusion, p [N, C, Ho, Wo] or None) as numpy."""
    Ho, Wo = case.out_hw
    lows, views = device_views(case, view_lows)
    y = torch.from_numpy(cases.labels(case) if labels is None else labels).to(DEV)
    cw = cases.class_weight(case)
    cw_d = torch.from_numpy(cw).to(DEV) if cw is not None else None
    work = torch.full((query("seg_tta_workspace_floats", case.N * Ho * Wo),), float("nan"), device=DEV)
    out4 = torch.full((4,), float("nan"), device=DEV)
    conf = torch.zeros((case.C, case.C), dtype=torch.int64, device=DEV)
    prob = torch.full((case.N, case.C, Ho, Wo), float("nan"), device=DEV) if want_prob else None
    call("seg_tta_upsample_eval", ctypes.addressof(views), len(lows), case.N, case.C, y.data_ptr(), Ho, Wo,
         case.ignore_index, cw_d.data_ptr() if cw_d is not None else None, 0 if case.reduction == "mean" else 1,
         work.data_ptr(), out4.data_ptr(), conf.data_ptr(), prob.data_ptr() if prob is not None else None, stream())
    torch.cuda.synchronize()
    return out4.cpu().numpy(), conf.cpu().numpy(), prob.cpu().numpy() if prob is not None else None


def run_classify(case, view_lows):
    """seg_tta_argmax_nearest -> (state rows [N*Ho*Wo, lds], p [N, C, Ho, Wo], labels, mask) as numpy; the state
    starts as NaN, four lanes wider than the logits' rows when those are wider than round4(C)."""
    Ho, Wo = case.out_hw
    Hf, Wf = case.frame_hw
    lows, views = device_views(case, view_lows)
    lds = (case.C + 3) // 4 * 4 + case.extra_ld
    state = torch.full((case.N * Ho * Wo, lds), float("nan"), device=DEV)
    labels = torch.full((case.N, Ho, Wo), 255, dtype=torch.uint8, device=DEV)
    mask = torch.full((case.N, Hf, Wf), 255, dtype=torch.uint8, device=DEV)
    call("seg_tta_argmax_nearest", ctypes.addressof(views), len(lows), case.N, case.C, Ho, Wo, state.data_ptr(), lds,
         case.min_conf, case.fallback, labels.data_ptr(), mask.data_ptr(), Hf, Wf, stream())
    torch.cuda.synchronize()
    rows = state.cpu().numpy()
    p = rows.reshape(case.N, Ho, Wo, lds)[..., :case.C].transpose(0, 3, 1, 2)
    return rows, p, labels.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_eval_matches_reference(case, record):
    want = cases.answer(case)
    y = cases.labels(case)
    out4, conf, p = run_eval(case, cases.lows(case))
    err = float(np.abs(p - want.p).max())
    excluded = float((~want.decided).mean())
    own = np.stack([ref.classify(s) for s in p])
    valid = y != case.ignore_index
    # the matrix is the bincount of the kernel's own classes, its total the valid count
    np.testing.assert_array_equal(conf, ref.confusion(own, y, case.C, case.ignore_index))
    assert conf.sum() == out4[3] == want.valid and out4[2] == 0
    # ... and those classes are the reference's wherever it is decided
    ok = want.decided & valid
    np.testing.assert_array_equal(own[ok], want.classes[ok])
    rel = abs(float(out4[0]) - want.loss) / max(abs(want.loss), 1e-30)
    record(case=case.name, kernel="seg_tta_upsample_eval", worst_abs_err=err, bound=TOL,
           worst_excluded_fraction=excluded, loss=float(out4[0]), loss_ref=want.loss, loss_rel_err=rel)
    print(f"{case.name}: worst |p - p_ref| {err:.3e} (bound {TOL:g}), excluded {excluded:.4f}, loss {out4[0]:.7g} "
          f"vs {want.loss:.7g} (rel {rel:.2e})")
    assert excluded <= 0.01
    assert err <= TOL, err
    assert abs(float(out4[0]) - want.loss) <= 1e-5 * abs(want.loss) + 1e-7
    assert abs(float(out4[1]) - want.D) <= 1e-6 * want.D
    # without the probability output: the same loss and matrix, bit for bit
    o2, c2, _ = run_eval(case, cases.lows(case), want_prob=False)
    assert o2.tobytes() == out4.tobytes() and np.array_equal(c2, conf)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_classify_matches_reference(case, record):
    want = cases.answer(case)
    rows, p, labels, mask = run_classify(case, cases.lows(case))
    err = float(np.abs(p - want.p).max())
    excluded = float((~want.decided).mean())
    for n in range(case.N):
        own = ref.classify(p[n], np.float32(case.min_conf), case.fallback)
        np.testing.assert_array_equal(labels[n], own)
        np.testing.assert_array_equal(mask[n], ref.to_frame(labels[n], case.frame_hw))
    np.testing.assert_array_equal(labels[want.decided], want.labels[want.decided])
    if case.min_conf > 0:
        assert 0.2 <= (labels == case.fallback).mean() <= 0.9
    # pad lanes of the written quads 0, the quads past them untouched
    r4 = (case.C + 3) // 4 * 4
    assert np.all(rows[:, case.C:r4] == 0) and np.isnan(rows[:, r4:]).all()
    record(case=case.name, kernel="seg_tta_argmax_nearest", worst_abs_err=err, bound=TOL,
           worst_excluded_fraction=excluded)
    print(f"{case.name}: worst |p - p_ref| {err:.3e} (bound {TOL:g}), excluded {excluded:.4f}")
    assert excluded <= 0.01
    assert err <= TOL, err


@pytest.mark.parametrize("name", ["scales6-weights-c19", "wide-rows-c32", "x2-hflip-c10"])
def test_two_runs_are_bitwise_equal(name):
    case = cases.BY_NAME[name]
    a, b = run_eval(case, cases.lows(case)), run_eval(case, cases.lows(case))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a, b = run_classify(case, cases.lows(case)), run_classify(case, cases.lows(case))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_probabilities_only():
    """NULL labels (and then a NULL matrix): p alone, bitwise the labelled run's, nothing counted."""
    case = cases.BY_NAME["scales6-weights-c19"]
    Ho, Wo = case.out_hw
    _, _, want = run_eval(case, cases.lows(case))
    lows, views = device_views(case, cases.lows(case))
    work = torch.empty(query("seg_tta_workspace_floats", case.N * Ho * Wo), device=DEV)
    out4 = torch.full((4,), float("nan"), device=DEV)
    prob = torch.full((case.N, case.C, Ho, Wo), float("nan"), device=DEV)
    call("seg_tta_upsample_eval", ctypes.addressof(views), len(lows), case.N, case.C, None, Ho, Wo, -100, None, 0,
         work.data_ptr(), out4.data_ptr(), None, prob.data_ptr(), stream())
    assert prob.cpu().numpy().tobytes() == want.tobytes()
    assert out4[2].item() == 0 and out4[3].item() == 0


def test_pad_lanes_are_left_alone():
    """The logits' pad lanes (1e30) never reach a result -- the reference comparison above runs on them -- and other
    values there change nothing, bit for bit."""
    case = cases.BY_NAME["wide-rows-c10"]
    lows = cases.lows(case)
    other = [lo.copy() for lo in lows]
    for lo in other:
        lo[..., case.C:] = np.nan
    a, b = run_eval(case, lows), run_eval(case, other)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a, b = run_classify(case, lows), run_classify(case, other)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def test_non_finite_logit_in_validation():
    """No special case: a NaN logit makes the loss NaN, and its pixels are still binned under some class."""
    case = cases.BY_NAME["x2-hflip-c10"]
    lows = [lo.copy() for lo in cases.lows(case)]
    lows[0][0, 3, 5, 2] = np.nan
    lows[1][1, 7, 15, 0] = np.inf
    out4, conf, p = run_eval(case, lows)
    assert np.isnan(out4[0]) and conf.sum() == out4[3] == cases.answer(case).valid and out4[2] == 0
    hit = np.isnan(p).any(axis=1)
    assert 2 <= hit.sum() <= 64 and np.abs(p - cases.answer(case).p)[~np.broadcast_to(hit[:, None], p.shape)].max() <= TOL


def test_out_of_range_label_is_counted():
    case = cases.BY_NAME["scales6-weights-c19"]
    y = cases.labels(case).copy()
    y[0, 0, :3] = case.C
    y[1, 5, 7] = -1
    out4, conf, _ = run_eval(case, cases.lows(case), labels=y)
    valid = (y != case.ignore_index) & (y >= 0) & (y < case.C)
    assert np.isnan(out4[0]) and out4[2] == 4 and out4[3] == valid.sum() == conf.sum()


@pytest.mark.parametrize("name", ["x2-hflip-c10", "c20-any"])
def test_predictor_rule_for_non_finite_views(name):
    """A view with a non-finite z at a pixel is left out there and the others renormalised; none left: 1/C."""
    case = cases.BY_NAME[name]
    lows = [lo.copy() for lo in cases.lows(case)]
    lows[0][0, 3, 5, 2] = np.nan
    lows[1][1, 7, 15, 0] = -np.inf
    want = cases.compute(case, lows, guarded=True)
    _, p, labels, mask = run_classify(case, lows)
    assert np.isfinite(p).all() and np.abs(p - want.p).max() <= TOL
    np.testing.assert_array_equal(labels[want.decided], want.labels[want.decided])
    changed = np.abs(want.p - cases.answer(case).p).max(axis=1) > 1e-3
    assert changed.any() and changed.sum() <= 64
    for lo, flip in zip(lows, cases.flips(case)):  # every view non-finite at the same place of image 0
        lo[0, 3, lo.shape[2] - 1 - 5 if flip else 5, 1] = np.nan
    _, p, labels, _ = run_classify(case, lows)
    none = ~np.isfinite(cases.compute(case, lows).p).all(axis=1) & \
        (cases.compute(case, lows, guarded=True).p[:, 0] == 1.0 / case.C)
    assert none[0].any() and not none[1].any()
    assert np.all(p.transpose(0, 2, 3, 1)[none] == np.float32(1) / np.float32(case.C)) and np.all(labels[none] == 0)


# ------------------------------------------------------------------------------------------- seg_tta_view_nchw
def _bilinear64(x, Hv, Wv):
    """F.interpolate(mode="bilinear", align_corners=False) of [N, C, H, W] in float64 (exact coordinates)."""
    def taps(n_out, n_in):
        src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = src - i0
        return i0, i1, 1.0 - l1, l1
    x = x.astype(np.float64)
    y0, y1, h0, h1 = taps(Hv, x.shape[2])
    x0, x1, w0, w1 = taps(Wv, x.shape[3])
    top = x[:, :, y0][:, :, :, x0] * w0 + x[:, :, y0][:, :, :, x1] * w1
    bot = x[:, :, y1][:, :, :, x0] * w0 + x[:, :, y1][:, :, :, x1] * w1
    return top * h0[None, None, :, None] + bot * h1[None, None, :, None]


@pytest.mark.parametrize("shape", [(2, 3, 32, 64, 24, 48), (2, 3, 32, 64, 40, 80), (1, 3, 24, 40, 48, 80),
                                   (1, 3, 17, 23, 9, 31), (2, 3, 32, 64, 32, 64)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("flip", [0, 1])
def test_view_kernel(shape, flip, record):
    """Against float64 bilinear.  The bound comes from the input: the rounding of the float32 source coordinate,
    Wv * 2^-23, times the largest difference between neighbours, plus 4 ulps of the largest magnitude for the
    blend itself."""
    N, C, H, W, Hv, Wv = shape
    x = np.random.Generator(np.random.PCG64([7, *shape])).normal(0, 1, (N, C, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    out = torch.full((N, C, Hv, Wv), float("nan"), device=DEV)
    call("seg_tta_view_nchw", xd.data_ptr(), N, C, H, W, out.data_ptr(), Hv, Wv, flip, stream())
    got = out.cpu().numpy()
    want = _bilinear64(x, Hv, Wv)
    if flip:
        want = want[..., ::-1]
    dmax = max(np.abs(np.diff(x, axis=2)).max(), np.abs(np.diff(x, axis=3)).max())
    bound = Wv * 2.0 ** -23 * dmax + 4 * np.spacing(np.float32(np.abs(x).max()))
    err = float(np.abs(got - want).max())
    record(kernel="seg_tta_view_nchw", shape=list(shape), flip=flip, worst_abs_err=err, bound=float(bound))
    print(f"view {shape} flip {flip}: worst error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if (H, W) == (Hv, Wv):  # a copy, or the mirror image
        assert np.array_equal(got, x[..., ::-1] if flip else x)


# ------------------------------------------------------------------------------------------- seg_preprocess_bgr_views
@pytest.mark.parametrize("geom", [(90, 160, 32, 64, 4), (61, 166, 24, 40, 8), (720, 1280, 128, 256, 4)],
                         ids=lambda g: "x".join(map(str, g)))
def test_preprocess_views_mirror_bitwise(geom):
    from seg_amd.infer import MEAN, STD
    Hf, Wf, H, W, ld = geom
    frame = torch.from_numpy(np.random.Generator(np.random.PCG64([9, *geom])).integers(0, 256, (Hf, Wf, 3),
                                                                                        dtype=np.uint8)).to(DEV)
    one = torch.full((H * W, ld), float("nan"), device=DEV)
    call("seg_preprocess_bgr", frame.data_ptr(), 1, Hf, Wf, frame.stride(0), one.data_ptr(), ld, H, W, *MEAN, *STD,
         stream())
    plain = one.view(H, W, ld)[..., :4]
    for copies, mask in ((1, 0), (1, 1), (2, 2), (3, 5)):
        out = torch.full((copies * H * W, ld), float("nan"), device=DEV)
        call("seg_preprocess_bgr_views", frame.data_ptr(), Hf, Wf, frame.stride(0), out.data_ptr(), ld, H, W, copies,
             mask, *MEAN, *STD, stream())
        got = out.view(copies, H, W, ld)
        for i in range(copies):
            want = torch.flip(plain, (1,)) if (mask >> i) & 1 else plain
            assert torch.equal(got[i, :, :, :4].view(torch.int32), want.view(torch.int32)), (copies, mask, i)
            assert torch.isnan(got[i, :, :, 4:]).all()
