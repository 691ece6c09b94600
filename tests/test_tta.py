"""CPU: test-time augmentation (seg_amd/tta.py) -- the option object and view sizes, the float64 restatement
(tests/tta_ref.py) against an independent torch float64 composition, the synthetic cases' undecided share,
the CPU definition of forward_tta / forward_metrics_tta / validate(tta=...) against compositions of the same
model's outputs, option errors, and the C ABI's argument validation (no GPU needed: it precedes any launch).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_cases as cases  # noqa: E402
import tta_ref as ref  # noqa: E402

import seg_amd  # noqa: E402
from seg_amd import LightUNet, MobileNetV2UNet, TTA, UNet, deterministic_init, view_shapes  # noqa: E402
from seg_amd.tta import MAX_VIEWS, SegTtaView, as_tta, make_view  # noqa: E402


# ------------------------------------------------------------------------------------------- the option object
def test_tta_views_and_weights():
    t = TTA()
    assert t.views() == [(1.0, False, 0.5), (1.0, True, 0.5)]
    assert as_tta("hflip").views() == t.views() and as_tta(None) is None and as_tta(t) is t
    t = TTA((0.5, 1.0, 2.0), hflip=True, weights=(1, 2, 1))
    assert [(s, f) for s, f, _ in t.views()] == [(0.5, False), (0.5, True), (1.0, False), (1.0, True), (2.0, False),
                                                 (2.0, True)]
    w = [w for _, _, w in t.views()]
    assert w == [0.125, 0.125, 0.25, 0.25, 0.125, 0.125]
    assert [w for _, _, w in TTA((0.75, 1.25), hflip=False, weights=(3, 1)).views()] == [0.75, 0.25]
    assert len(TTA((0.5, 0.75, 1, 1.25), hflip=True).views()) == MAX_VIEWS == 8


@pytest.mark.parametrize("kwargs", [
    dict(scales=()), dict(scales=(0.4,)), dict(scales=(2.5,)), dict(scales=("1",)), dict(scales=(True,)),
    dict(scales=(1.0, float("nan"))), dict(hflip=1), dict(weights=(1, 1)), dict(scales=(1, 1.5), weights=(1,)),
    dict(scales=(1.0, 1.0)), dict(scales=(0.75, 1, 0.75), hflip=False), dict(weights=(0,)), dict(weights=(-1.0,)), dict(weights=(float("inf"),)), dict(weights=(float("nan"),)),
    dict(scales=(0.5, 0.75, 1, 1.25, 1.5), hflip=True), dict(scales=tuple(0.5 + 0.1 * k for k in range(9)), hflip=False),
])
def test_tta_rejects(kwargs):
    with pytest.raises(ValueError):
        TTA(**kwargs)


def test_as_tta_rejects():
    for bad in ("flip", 1.0, ("hflip",), True):
        with pytest.raises(ValueError):
            as_tta(bad)


def test_view_shapes():
    mob, unet = MobileNetV2UNet(3), UNet(3, base_filters=4)
    t = TTA((0.75, 1, 1.25))
    assert [(h, w, f) for h, w, f, _ in view_shapes(mob, 128, 256, t)] == [
        (96, 192, False), (96, 192, True), (128, 256, False), (128, 256, True), (160, 320, False), (160, 320, True)]
    assert sum(w for *_, w in view_shapes(mob, 128, 256, t)) == pytest.approx(1.0, abs=1e-15)
    with pytest.raises(ValueError, match="both give"):
        view_shapes(mob, 64, 128, TTA((0.75, 1)))  # 64 * 0.75 / 32 = 1.5 -> 2: 64 again
    # the divisor is the model's: 8 for the UNets, where the same scales stay apart
    assert [(h, w) for h, w, _, _ in view_shapes(unet, 64, 128, TTA((0.75, 1), hflip=False))] == [(48, 96), (64, 128)]
    assert [(h, w) for h, w, _, _ in view_shapes(LightUNet(8), 32, 32, TTA((0.75, 1, 1.25), hflip=False))] == [
        (24, 24), (32, 32), (40, 40)]
    assert view_shapes(mob, 32, 32, TTA((0.5,), hflip=False))[0][:2] == (32, 32)  # max(1, .): never 0
    assert view_shapes(mob, 128, 256, "hflip") == [(128, 256, False, 0.5), (128, 256, True, 0.5)]
    with pytest.raises(TypeError):
        view_shapes(torch.nn.Conv2d(3, 3, 1), 64, 64, "hflip")


def test_make_view_cpu():
    x = torch.randn(2, 3, 16, 24)
    assert make_view(x, 16, 24, False) is x  # a scale that keeps the size does no resize
    assert torch.equal(make_view(x, 16, 24, True), torch.flip(x, (-1,)))
    want = torch.flip(F.interpolate(x, (24, 40), mode="bilinear", align_corners=False), (-1,))
    assert torch.equal(make_view(x, 24, 40, True), want)


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", [c for c in cases.CASES if c.name != "grid-stride-c3"], ids=lambda c: c.name)
def test_restatement_against_torch_float64(case):
    """tta_ref.probabilities against F.interpolate(align_corners=True) + flip + softmax + weighted mean in float64.
    The restatement forms its source coordinates in float32 (as the kernels do), torch in float64: a coordinate
    differs by at most one float32 rounding of a value below max(Hl, Wl), which moves z by at most that times the
    largest difference between neighbouring logits, per axis; softmax and the convex mean do not enlarge it."""
    view_lows = cases.lows(case)
    got = cases.answer(case).p
    Ho, Wo = case.out_hw
    w = ref.normalised(cases.weights(case))
    want = torch.zeros((case.N, case.C, Ho, Wo), dtype=torch.float64)
    bound = 0.0
    for low, flip, wk in zip(view_lows, cases.flips(case), w):
        z = torch.from_numpy(low[..., :case.C].astype(np.float64)).permute(0, 3, 1, 2)
        dz = max(float((z[:, :, 1:] - z[:, :, :-1]).abs().max()) if z.shape[2] > 1 else 0.0,
                 float((z[:, :, :, 1:] - z[:, :, :, :-1]).abs().max()) if z.shape[3] > 1 else 0.0)
        bound = max(bound, 2 * max(z.shape[2:]) * 2.0 ** -23 * dz)
        z = F.interpolate(z, (Ho, Wo), mode="bilinear", align_corners=True)
        if flip:
            z = torch.flip(z, (-1,))
        want += wk * torch.softmax(z, dim=1)
    err = float(np.abs(got - want.numpy()).max())
    assert err <= bound + 1e-12, (err, bound)
    assert np.allclose(got.sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_cases_are_decided(case):
    """At most 1 % of a case's pixels are undecided (the project's cap), so the GPU test's label comparison
    means something; the threshold case paints a real share of its pixels."""
    a = cases.answer(case)
    assert (~a.decided).mean() <= 0.01, (~a.decided).mean()
    assert np.isfinite(a.loss) and a.valid > 0
    assert 0.05 <= (cases.labels(case) == case.ignore_index).mean() <= 0.15
    if case.min_conf > 0:
        assert 0.2 <= (a.labels == case.fallback).mean() <= 0.9


def test_grid_stride_case_goes_round_twice():
    case = cases.BY_NAME["grid-stride-c3"]
    px = case.N * case.out_hw[0] * case.out_hw[1]
    assert 2048 * 256 < px <= 2 * 2048 * 256 and 8192 * 64 < px


def test_guarded_rule_of_the_restatement():
    """A NaN in one view leaves that view out where it reaches; in every view: 1/C."""
    case = cases.BY_NAME["x2-hflip-c10"]
    lows = [lo.copy() for lo in cases.lows(case)]
    lows[0][0, 3, 5, 2] = np.nan
    a = cases.compute(case, lows, guarded=True)
    one = [cases.channel_first(case, lows[1], 0)]
    alone = ref.probabilities_guarded(one, [True], [1.0], case.out_hw)
    hit = ~np.isfinite(ref.view_logits(cases.channel_first(case, lows[0], 0), False, case.out_hw)).all(axis=0)
    assert 1 <= hit.sum() <= 16 and np.isfinite(a.p).all()
    assert np.array_equal(a.p[0][:, hit], alone[:, hit])
    assert np.abs(a.p[0][:, ~hit] - cases.answer(case).p[0][:, ~hit]).max() == 0
    lows[1][0, :, :, 0] = np.inf
    assert np.all(cases.compute(case, lows, guarded=True).p[0][:, hit] == 1.0 / case.C)


# ------------------------------------------------------------------------------------------- the CPU definition
def _labels(N, C, H, W, seed, ignore_index=-100):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (N, H, W), generator=g)
    y[torch.rand((N, H, W), generator=g) < 0.1] = ignore_index
    return y


@pytest.fixture(scope="module")
def mob():
    model = deterministic_init(MobileNetV2UNet(5), seed=3).eval()
    x = torch.randn(1, 3, 128, 256, generator=torch.Generator().manual_seed(1))
    return model, x


def test_cpu_hflip_matches_the_models_own_outputs(mob):
    model, x = mob
    with torch.no_grad():
        want = 0.5 * torch.softmax(model(x), 1) + 0.5 * torch.flip(torch.softmax(model(torch.flip(x, (-1,))), 1), (-1,))
        p = model.forward_tta(x, "hflip")
    assert p.shape == (1, 5, 128, 256) and p.dtype == torch.float32
    assert float((p - want).abs().max()) <= 1e-6
    y = _labels(1, 5, 128, 256, 2)
    w = torch.tensor([0.5, 1.0, 2.0, 1.5, 0.7])
    for reduction in ("mean", "sum"):
        conf = torch.zeros((5, 5), dtype=torch.int64)
        loss = model.forward_metrics_tta(x, y, conf, "hflip", weight=w, reduction=reduction)
        ref_loss = F.nll_loss(torch.log(want), y, weight=w, reduction=reduction)
        assert abs(loss.item() - ref_loss.item()) <= 1e-5 * abs(ref_loss.item())
        keep = y != -100
        assert int(conf.sum()) == int(keep.sum())
        assert torch.equal(conf, torch.bincount(y[keep] * 5 + p.argmax(1)[keep], minlength=25).reshape(5, 5))


def test_cpu_multi_scale_matches_the_restatement(mob):
    """TTA((0.75, 1)) at 128x256: the 96x192 view's logits (48x96) reach the 128x256 grid by ONE interpolation."""
    from seg_amd.export import torch_low_logits
    model, x = mob
    tta = TTA((0.75, 1.0), weights=(1, 3))
    shapes = view_shapes(model, 128, 256, tta)
    with torch.no_grad():
        lows = [torch_low_logits(model, make_view(x, h, w, f))[0].numpy() for h, w, f, _ in shapes]
        p = model.forward_tta(x, tta)[0].numpy()
    assert [lo.shape[1:] for lo in lows] == [(48, 96), (48, 96), (64, 128), (64, 128)]
    want = ref.probabilities(lows, [s[2] for s in shapes], [s[3] for s in shapes], (128, 256))
    assert np.abs(p - want).max() <= 1e-5


def test_cpu_light_unet():
    model = deterministic_init(LightUNet(8), seed=5).eval()
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    tta = TTA((0.75, 1, 1.25))
    p = model.forward_tta(x, tta)
    assert p.shape == (1, 1, 32, 32) and float((p - 1).abs().max()) <= 1e-6  # one class
    conf = torch.zeros((1, 1), dtype=torch.int64)
    y = _labels(1, 1, 32, 32, 6)
    loss = model.forward_metrics_tta(x, y, conf, tta)
    assert abs(loss.item()) <= 1e-6 and int(conf[0, 0]) == int((y == 0).sum())


def test_cpu_unet_scales_against_the_restatement():
    from seg_amd.export import torch_low_logits
    model = deterministic_init(UNet(4, base_filters=8), seed=7).eval()
    x = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(8))
    tta = TTA((0.75, 1, 1.25), hflip=True, weights=(1, 2, 1))
    shapes = view_shapes(model, 32, 48, tta)
    with torch.no_grad():
        lows = [torch_low_logits(model, make_view(x, h, w, f)).numpy() for h, w, f, _ in shapes]
        p = model.forward_tta(x, tta).numpy()
    for n in range(2):
        want = ref.probabilities([lo[n] for lo in lows], [s[2] for s in shapes], [s[3] for s in shapes], (32, 48))
        assert np.abs(p[n] - want).max() <= 1e-5


def _loader(model_c, n_batches, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(N, 3, H, W, generator=g), _labels(N, model_c, H, W, seed + k)) for k in range(n_batches)]


def test_validate_identity_tta_is_plain_validate(mob):
    model, _ = mob
    loader = _loader(5, 2, 1, 64, 64, 11)
    crit = torch.nn.CrossEntropyLoss()
    plain = seg_amd.validate(model, loader, crit, "cpu", progress=False)
    ident = seg_amd.validate(model, loader, crit, "cpu", progress=False, tta=TTA(scales=(1,), hflip=False))
    assert torch.equal(plain["confusion"], ident["confusion"])
    assert abs(plain["loss"] - ident["loss"]) <= 1e-5 * abs(plain["loss"])
    assert plain["miou"] == ident["miou"]


def test_validate_tta_sums_batches_and_takes_the_hard_term(mob):
    model, _ = mob
    loader = _loader(5, 2, 1, 64, 64, 21)
    w = torch.tensor([0.5, 1.0, 2.0, 1.5, 0.7])
    losses, conf = [], torch.zeros((5, 5), dtype=torch.int64)
    for x, y in loader:
        losses.append(model.forward_metrics_tta(x, y, conf, "hflip", weight=w).item())
    for crit in (torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1), seg_amd.SegLoss(dice=0.5, weight=w),
                 seg_amd.OhemCELoss(thresh=0.7, min_kept=100, weight=w)):
        out = seg_amd.validate(model, loader, crit, "cpu", progress=False, tta="hflip")
        assert out["loss"] == sum(losses) / 2, type(crit).__name__
        assert torch.equal(out["confusion"], conf)
    with pytest.raises(IndexError):
        bad = [(loader[0][0], loader[0][1].clone().fill_(7))]
        seg_amd.validate(model, bad, torch.nn.CrossEntropyLoss(), "cpu", progress=False, tta="hflip")


def test_option_errors(mob):
    model, _ = mob
    loader = _loader(5, 1, 1, 64, 64, 31)
    with pytest.raises(ValueError):
        seg_amd.validate(model, loader, torch.nn.CrossEntropyLoss(), "cpu", progress=False, tta="flip")
    with pytest.raises(ValueError):  # reduction "none" is no fused criterion
        seg_amd.validate(model, loader, torch.nn.CrossEntropyLoss(reduction="none"), "cpu", progress=False, tta="hflip")
    with pytest.raises(ValueError):
        seg_amd.validate(model, loader, torch.nn.MSELoss(), "cpu", progress=False, tta="hflip")
    with pytest.raises(ValueError):
        seg_amd.validate(torch.nn.Conv2d(3, 5, 1), loader, torch.nn.CrossEntropyLoss(), "cpu", progress=False,
                         tta="hflip")
    with pytest.raises(ValueError, match="both give"):
        seg_amd.validate(model, loader, torch.nn.CrossEntropyLoss(), "cpu", progress=False, tta=TTA((0.75, 1)))
    with pytest.raises(ValueError):
        model.forward_metrics_tta(loader[0][0], loader[0][1], torch.zeros((5, 5), dtype=torch.int64), "hflip",
                                  reduction="none")
    # Predictor: the options are checked before anything touches a device
    with pytest.raises(ValueError, match="temporal"):
        seg_amd.Predictor(model, tta="hflip", temporal=0.5)
    with pytest.raises(ValueError):
        seg_amd.Predictor(model, tta="mirror")
    with pytest.raises(ValueError):
        seg_amd.Predictor(model, tta="hflip", tta_batch=1)
    with pytest.raises(ValueError, match="f16"):
        seg_amd.Predictor(model, tta="hflip", tta_batch=True, math="f16")


# ------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    from seg_amd import _lib
    from seg_amd.build import build
    build()
    return _lib.lib()


def _views(n, ld=12, weight=1.0, low=0x1000, H=8, W=16):
    arr = (SegTtaView * max(n, 1))()
    for v in arr:
        v.low, v.ld, v.H, v.W, v.flip, v.weight = low, ld, H, W, 0, weight
    return arr


def test_abi_rejects_before_any_launch(lib):
    """hipErrorInvalidValue (1) on each of the documented arguments, on a machine without a GPU: nothing is launched."""
    assert ctypes.sizeof(SegTtaView) == 32
    def rc_eval(views, n=2, C=10, reduction=0, conf=0x2000):
        return lib.seg_tta_upsample_eval(ctypes.addressof(views) if views is not None else None, n, 2, C, 0x3000, 16,
                                         32, -100, None, reduction, 0x4000, 0x5000, conf, None, None)

    def rc_pred(views, n=2, C=10):
        return lib.seg_tta_argmax_nearest(ctypes.addressof(views) if views is not None else None, n, 1, C, 16, 32,
                                          0x6000, 12, 0.0, 0, 0x7000, 0x8000, 45, 80, None)

    for rc in (rc_eval, rc_pred):
        assert rc(_views(2), n=0) == 1 and rc(_views(8), n=9) == 1 and rc(None) == 1   # nviews outside 1..8
        assert rc(_views(2, low=None)) == 1                                              # a NULL view pointer
        assert rc(_views(2, ld=10)) == 1 and rc(_views(2, ld=8)) == 1                    # ld % 4, ld < C
        for w in (0.0, -1.0, float("inf"), float("nan")):
            assert rc(_views(2, weight=w)) == 1                                          # weights positive and finite
        assert rc(_views(2), C=0) == 1
    # probabilities only (NULL labels) needs the probability output
    assert lib.seg_tta_upsample_eval(ctypes.addressof(_views(2)), 2, 2, 10, None, 16, 32, -100, None, 0, 0x4000, 0x5000,
                                     None, None, None) == 1
    assert lib.seg_preprocess_bgr_views(None, 720, 1280, 3840, 0x2000, 4, 128, 256, 2, 2, 0, 0, 0, 1, 1, 1, None) == 1
    assert lib.seg_preprocess_bgr_views(0x1000, 720, 1280, 3840, None, 4, 128, 256, 2, 2, 0, 0, 0, 1, 1, 1, None) == 1
    assert rc_eval(_views(2), reduction=2) == 1 and rc_eval(_views(2), conf=None) == 1 and rc_eval(_views(2, ld=36), C=33) == 1
    assert rc_pred(_views(2, ld=256), C=256) == 1
    assert lib.seg_tta_view_nchw(None, 1, 3, 8, 8, 0x1000, 8, 8, 0, None) == 1
    assert lib.seg_tta_view_nchw(0x1000, 1, 3, 8, 8, 0x2000, 0, 8, 0, None) == 1
    assert lib.seg_preprocess_bgr_views(0x1000, 720, 1280, 1280, 0x2000, 4, 128, 256, 2, 2, 0, 0, 0, 1, 1, 1, None) == 1
    assert lib.seg_preprocess_bgr_views(0x1000, 720, 1280, 3840, 0x2000, 4, 128, 256, 9, 0, 0, 0, 0, 1, 1, 1, None) == 1
    assert lib.seg_preprocess_bgr_views(0x1000, 720, 1280, 3840, 0x2000, 4, 128, 256, 2, 4, 0, 0, 0, 1, 1, 1, None) == 1
    assert lib.seg_tta_workspace_floats(1) == 5 and lib.seg_tta_workspace_floats(1 << 30) == 5 * 2048
