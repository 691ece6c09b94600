"""GPU: test-time augmentation through the models, validate() and the Predictor.

The reference (tests/tta_ref.py, float64) is evaluated on the GPU model's OWN per-view forward_low_logits, so the
comparison isolates what the ensemble adds -- the view kernel's output feeds both sides, the forwards are the same
launches -- at the kernel-level bounds of test_gpu_tta.py: |p - p_ref| <= 1e-5, the classes wherever the
reference is decided, the matrix exactly the bincount of the kernel's own classes, the loss within 1e-5 relative.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as ref  # noqa: E402

import seg_amd  # noqa: E402
from oracle import cvresize  # noqa: E402
from seg_amd import LightUNet, MobileNetV2UNet, TTA, UNet, deterministic_init, view_shapes  # noqa: E402
from seg_amd.engine import bad_label_count, set_conv_math  # noqa: E402
from seg_amd.infer import Predictor  # noqa: E402
from seg_amd.tta import make_view  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5

CONFIGS = {
    "mobilenet": (lambda: MobileNetV2UNet(10), (2, 64, 128), TTA((1, 1.5)), 10),
    "lightunet": (lambda: LightUNet(16), (1, 32, 32), TTA((0.75, 1, 1.25)), 1),
}


def build(name, math):
    make, (N, H, W), tta, C = CONFIGS[name]
    model = deterministic_init(make(), seed=5, random_running_stats=True).to(DEV).eval()
    set_conv_math(model, math)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 3, H, W, generator=g).to(DEV)
    y = torch.randint(0, C, (N, H, W), generator=g)
    y[torch.rand((N, H, W), generator=g) < 0.1] = -100
    return model, x, y.to(DEV), tta, C


def reference(model, x, tta, C):
    """float64 p [N, C, H, W] from the model's own per-view low-resolution logits."""
    N, _, H, W = x.shape
    shapes = view_shapes(model, H, W, tta)
    lows = [model.forward_low_logits(make_view(x, hv, wv, f))[..., :C].permute(0, 3, 1, 2).cpu().numpy()
            for hv, wv, f, _ in shapes]
    return np.stack([ref.probabilities([lo[n] for lo in lows], [s[2] for s in shapes], [s[3] for s in shapes], (H, W))
                     for n in range(N)])


@pytest.mark.parametrize("math", ["f32", "bf16io"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_tta_and_metrics_match_reference(name, math, record):
    model, x, y, tta, C = build(name, math)
    want = reference(model, x, tta, C)
    p = model.forward_tta(x, tta)
    assert p.shape == (x.shape[0], C, x.shape[2], x.shape[3]) and p.dtype == torch.float32
    got = p.cpu().numpy()
    err = float(np.abs(got - want).max())
    decided = np.stack([ref.decided(s) for s in want])
    own = np.stack([ref.classify(s) for s in got])
    np.testing.assert_array_equal(own[decided], np.stack([ref.classify(s) for s in want])[decided])
    w = torch.linspace(0.5, 2.0, C, device=DEV) if C > 1 else None
    yn = y.cpu().numpy()
    for weight, reduction in ((None, "mean"), (w, "sum")):
        conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
        loss = model.forward_metrics_tta(x, y, conf, tta, weight=weight, reduction=reduction)
        assert int(bad_label_count(model).item()) == 0
        want_loss, _, valid = ref.nll(want, yn, -100, None if weight is None else weight.cpu().numpy(), reduction)
        np.testing.assert_array_equal(conf.cpu().numpy(), ref.confusion(own, yn, C))
        assert int(conf.sum()) == valid
        assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss) + 1e-7, (loss.item(), want_loss)
    record(model=name, math=math, worst_abs_err=err, bound=TOL, worst_excluded_fraction=float((~decided).mean()))
    print(f"{name} {math}: worst |p - p_ref| {err:.3e} (bound {TOL:g}), excluded {(~decided).mean():.4f}")
    assert err <= TOL, err


@pytest.mark.parametrize("math", ["f32", "bf16io"])
def test_identity_tta_is_plain_forward_metrics(math):
    model, x, y, _, C = build("mobilenet", math)
    a = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    b = torch.zeros_like(a)
    plain = model.forward_metrics(x, y, a)
    ident = model.forward_metrics_tta(x, y, b, TTA(scales=(1,), hflip=False))
    assert torch.equal(a, b)
    assert abs(plain.item() - ident.item()) <= 1e-5 * abs(plain.item())


def test_validate_sums_the_batches_and_raises_on_a_bad_label():
    model, x, y, _, C = build("mobilenet", "f32")
    x2 = torch.flip(x, (0, 2))
    y2 = torch.flip(y, (0, 1))
    loader = [(x, y), (x2, y2)]
    conf = torch.zeros((C, C), dtype=torch.int64, device=DEV)
    losses = [model.forward_metrics_tta(xx, yy, conf, "hflip").item() for xx, yy in loader]
    model.train()
    out = seg_amd.validate(model, loader, torch.nn.CrossEntropyLoss(), DEV, progress=False, tta="hflip")
    assert model.training  # the mode is restored
    model.eval()
    assert out["loss"] == sum(losses) / 2
    assert torch.equal(out["confusion"], conf.cpu())
    plain = seg_amd.validate(model, loader, torch.nn.CrossEntropyLoss(), DEV, progress=False)
    assert not torch.equal(plain["confusion"], out["confusion"])  # the ensemble is really on
    assert int(plain["confusion"].sum()) == int(out["confusion"].sum())
    bad = y.clone()
    bad[0, 0, 0] = C
    with pytest.raises(IndexError):
        seg_amd.validate(model, [(x, y), (x, bad)], torch.nn.CrossEntropyLoss(), DEV, progress=False, tta="hflip")


# ------------------------------------------------------------------------------------------- Predictor
SIZE = (64, 32)  # cv2 order: the model sees 32 x 64
FHW = (61, 166)


def frame(h, w, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.linspace(0, 6, h), np.linspace(0, 9, w), indexing="ij")
    base = 127.5 + 100 * np.sin(yy)[..., None] * np.cos(xx[..., None] + np.arange(3))
    return np.clip(base + g.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def unet():
    return deterministic_init(UNet(10, 16), seed=11, random_running_stats=True).to(DEV)


def view_lows(pred):
    """The predictor's own per-view low-resolution logits [C, Hl, Wl], in view order."""
    out = []
    for rt, prog, n, _ in pred._tta_groups:
        lo = prog.logits
        rows = rt.bufs[lo.buf].view(-1, lo.ld)[:, lo.off:lo.off + lo.C].float().cpu().numpy()
        out += list(rows.reshape(n, lo.H, lo.W, lo.C).transpose(0, 3, 1, 2))
    return out


@pytest.mark.parametrize("tta,batch,math", [("hflip", True, "f32"), ("hflip", False, "f32"),
                                            (TTA((0.75, 1, 1.25), weights=(1, 2, 1)), True, "f32"),
                                            ("hflip", None, "f16"), (TTA((0.75, 1)), False, "f16")],
                         ids=["hflip-batch2", "hflip-two-runs", "scales", "f16-hflip", "f16-scales"])
def test_predictor_matches_reference_on_its_own_logits(unet, tta, batch, math, record):
    pred = Predictor(unet, frame_hw=FHW, target_size=SIZE, tta=tta, tta_batch=batch, min_confidence=0.5,
                     fallback_class=9, math=math)
    shapes = view_shapes(unet, 32, 64, tta)
    assert len(pred._tta_groups) == (len(shapes) // 2 if batch else len(shapes))  # f16: a run per view
    mask = pred(frame(*FHW, 3)).cpu().numpy()
    p = pred.probabilities()[0].cpu().numpy()
    want = ref.probabilities_guarded(view_lows(pred), [s[2] for s in shapes], [s[3] for s in shapes], (32, 64))
    err = float(np.abs(p - want).max())
    decided = ref.decided(want, 0.5)
    labels = ref.classify(p, np.float32(0.5), 9)
    np.testing.assert_array_equal(labels[decided], ref.classify(want, 0.5, 9)[decided])
    np.testing.assert_array_equal(mask, ref.to_frame(labels, FHW))
    np.testing.assert_array_equal(pred.confidence().cpu().numpy(), p.max(axis=0))
    record(tta=repr(tta), batch=batch, worst_abs_err=err, bound=TOL, worst_excluded_fraction=float((~decided).mean()))
    print(f"Predictor {tta!r} batch {batch}: worst |p - p_ref| {err:.3e}, excluded {(~decided).mean():.4f}, "
          f"fallback share {(labels == 9).mean():.3f}")
    assert err <= TOL, err


def test_predictor_flip_pair_as_one_batch_or_two_runs(unet):
    """The batch-2 forward and the two batch-1 forwards see the same two images: the masks agree but for near ties."""
    a = Predictor(unet, frame_hw=FHW, target_size=SIZE, tta="hflip", tta_batch=True)
    b = Predictor(unet, frame_hw=FHW, target_size=SIZE, tta="hflip", tta_batch=False)
    f = frame(*FHW, 4)
    assert (a(f) != b(f)).float().mean().item() <= 0.01
    plain = Predictor(unet, frame_hw=FHW, target_size=SIZE)
    assert (a(f) != plain(f)).float().mean().item() > 0.001  # the ensemble is really on


def test_predictor_graph_equals_eager_refresh_and_overlay(unet):
    model = deterministic_init(UNet(10, 16), seed=11, random_running_stats=True).to(DEV)
    g = Predictor(model, frame_hw=FHW, target_size=SIZE, tta="hflip", overlay=True)
    e = Predictor(model, frame_hw=FHW, target_size=SIZE, tta="hflip", graph=False)
    assert g.graph is not None and e.graph is None
    for seed in (3, 4):
        f = frame(*FHW, seed)
        assert torch.equal(g(f), e(f))
        assert torch.equal(g.probabilities(), e.probabilities())
    np.testing.assert_array_equal(g.mask.cpu().numpy(),
                                  cvresize.class_mask(g.probabilities().cpu().numpy(), FHW))
    result, found = g.annotate(f)
    assert tuple(result.shape) == (*FHW, 3) and result.dtype == torch.uint8 and "cars" in found
    before = g.mask.clone()
    with torch.no_grad():
        model.sem_out.conv[3].weight.mul_(-1.0)
    assert torch.equal(g(f), before)  # the folded weights are the old ones until refresh()
    g.refresh()
    e.refresh()
    after = g(f)
    assert (after != before).float().mean().item() > 0.05 and torch.equal(after, e(f))


def test_predictor_option_errors(unet):
    with pytest.raises(ValueError, match="temporal"):
        Predictor(unet, frame_hw=FHW, target_size=SIZE, tta="hflip", temporal=0.5)
    with pytest.raises(ValueError, match="f16"):
        Predictor(unet, frame_hw=FHW, target_size=SIZE, tta="hflip", tta_batch=True, math="f16")
    with pytest.raises(ValueError):
        Predictor(unet, frame_hw=FHW, target_size=SIZE, tta=TTA((0.9, 1)))  # 32 * 0.9 / 8 rounds to 32 again
    pred = Predictor(unet, frame_hw=FHW, target_size=SIZE, tta="hflip", graph=False)
    with pytest.raises(RuntimeError):
        pred.reset()
    with pytest.raises(RuntimeError):
        pred.logits()
