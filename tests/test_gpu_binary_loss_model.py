"""GPU: a seg_amd.BinarySegLoss through one-logit models -- compute_loss / validate / train_one_epoch take the fused
path for it (seg_bce_*), that path agrees with the same engine's logits path (criterion(model(x), t): full-resolution
logits, BinarySegLoss's torch forward), and Predictor(threshold=) writes the thresholded mask.  The shape of
tests/test_gpu_seg_loss_model.py.

Gradients: the head's weight and bias within 1e-4 (the project's figure); every parameter with a gradient to speak of
(the `real` filter of tests/test_gpu_seg_loss_model.py) within twice a yardstick measured in the same test, the worst
fused-vs-logits spread of MobileNetV2UNet(10) under plain nn.CrossEntropyLoss at the same input shape -- rounding
noise below the low-resolution logit gradient.  Both numbers go through `record`.  The assertion is over `real`
only: a parameter whose gradient is rounding noise in both paths (BatchNorm-shadowed conv biases) has no relative
error to speak of, as in the existing test.

Measured on an MI355X (profiles/binary_parity.jsonl): the yardstick is 1.73e-4 over the parameters with a gradient and
1.10 over all of them (pure noise).  LightUNet: worst 1.9e-6 (47 of 62 parameters have a gradient), head 7.6e-8 / 0.
MobileNetV2UNet(1): 2.50e-4 over the 178 of 194 with a gradient (bound 3.46e-4), head 2.2e-7 / 3.1e-7; over all 194
it is 1.06 against the yardstick's 1.10 -- the noise parameters, which is why the assertion is over `real`.  bf16io:
the two losses agree to 2e-7 and the head's gradients bit for bit (the low-resolution gradient is rounded to bf16
once, behind either path).  A fused step allocates exactly one full-resolution plane less than the logits path (the
logits; the one-float-per-pixel gradient plane stands where the logits path has the logits' gradient).
"""
import numpy as np
import pytest
import torch
from torch import nn

from seg_amd import (Adam, BinarySegLoss, LightUNet, MobileNetV2UNet, Predictor, engine, train_one_epoch, validate)
from seg_amd import _lib
from seg_amd.detinit import deterministic_init, synthetic_batch
from seg_amd.losses import logit_threshold
from seg_amd.metrics import binary_summary
from seg_amd.train import compute_loss, fused_loss_options

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 1e-4
MAX_LEFT_OUT = 0.005
KINDS = ["light", "mnv2"]
OPTION_SETS = [dict(pos_weight=2.5), dict(focal_gamma=0.5), dict(focal_gamma=2.0), dict(bce=0.0, dice=1.0),
               dict(bce=0.6, dice=1.4, focal_gamma=1.5, pos_weight=2.5, dice_smooth=0.5)]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def make(kind="mnv2", seed=1, train=False, conv_math="f32"):
    net = MobileNetV2UNet(1) if kind == "mnv2" else LightUNet()
    m = deterministic_init(net, seed=seed, random_running_stats=True).to(DEV)
    engine.set_conv_math(m, conv_math)
    return m.train() if train else m.eval()


def batch(n=2, seed=7):
    """2 x 3 x 64 x 64, labels in {0, 1}, three rows ignored."""
    x, y = synthetic_batch(n, 64, 64, 2, seed=seed)
    y[0, :3] = -100
    return x.to(DEV), y.to(DEV)


def grads_of(model, loss_fn):
    model.zero_grad(set_to_none=True)
    loss = loss_fn()
    loss.backward()
    return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


class Unfused(BinarySegLoss):
    """A forward of its own: fused_loss_options gives None, so the criterion runs on the full-resolution logits."""

    def forward(self, logits, target):
        return super().forward(logits, target)


@pytest.mark.parametrize("kind", KINDS)
def test_compute_loss_takes_the_fused_path(kind):
    model = make(kind)
    x, t = batch()
    assert engine.bad_label_count(model) is None
    for kw in OPTION_SETS:
        crit = BinarySegLoss(**kw)
        with torch.no_grad():
            loss = compute_loss(model, crit, x, t)
            assert engine.bad_label_count(model) is not None  # the logits path clears it
            assert engine.bad_label_count(model).item() == 0
            ref = crit(model(x), t)
            assert engine.bad_label_count(model) is None
        assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (kw, loss.item(), ref.item())
    # [N, 1, H, W] bool targets, and another ignore_index
    crit = BinarySegLoss(dice=1.0, ignore_index=255)
    t8 = torch.where(t == -100, torch.full_like(t, 255), t).to(torch.uint8).unsqueeze(1)
    with torch.no_grad():
        a, b = compute_loss(model, crit, x, t8), BinarySegLoss(dice=1.0)(model(x), t)
    assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item())
    # neither the full-resolution logits nor their gradient: with its plan recorded, a fused training step allocates
    # at least one full-resolution logits tensor less than the same step on the logits path
    full = x.shape[0] * 1 * x.shape[2] * x.shape[3] * 4
    tm = make(kind, train=True)
    crit = BinarySegLoss(dice=1.0, focal_gamma=2.0)
    grown = {}
    for name, fn in (("fused", lambda: compute_loss(tm, crit, x, t)), ("logits", lambda: crit(tm(x), t))):
        for k in range(2):  # record, then measure a replay
            tm.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn().backward()
            torch.cuda.synchronize()
            grown[name] = torch.cuda.max_memory_allocated() - base
    print(kind, "a step allocates", grown, "bytes; full-resolution logits", full)
    assert grown["fused"] + full <= grown["logits"], (grown, full)


def plain_yardstick(x):
    """The worst fused-vs-logits spread of MobileNetV2UNet(10) under plain cross-entropy at x's shape, over all
    parameters and over those with a gradient to speak of."""
    model = deterministic_init(MobileNetV2UNet(10), seed=1, random_running_stats=True).to(DEV).train()
    _, y = synthetic_batch(x.shape[0], x.shape[2], x.shape[3], 10, seed=7)
    y[0, :3] = -100
    y = y.to(DEV)
    plain = nn.CrossEntropyLoss()
    _, gf = grads_of(model, lambda: compute_loss(model, plain, x, y))
    _, gl = grads_of(model, lambda: plain(model(x), y))
    plain_rel = {k: rel(gf[k], gl[k]) for k in gf}
    top = max(float(g.norm()) for g in gl.values())
    real = [k for k in gl if float(gl[k].norm()) > 1e-6 * top]
    return max(plain_rel.values()), max(plain_rel[k] for k in real)


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_fused_against_logits_path(kind, record):
    # train(): the engine has no backward through eval-mode BatchNorm; the forward is the same launches in both paths
    model = make(kind, train=True)
    x, t = batch()
    last = [m for m in model.modules() if isinstance(m, nn.Conv2d)][-1]
    names = {id(p): k for k, p in model.named_parameters()}
    worst, worst_real = plain_yardstick(x)
    crit = BinarySegLoss(bce=0.6, dice=1.4, focal_gamma=1.5, pos_weight=2.5, dice_smooth=0.5)
    lf, wf = grads_of(model, lambda: compute_loss(model, crit, x, t))
    ll, wl = grads_of(model, lambda: crit(model(x), t))
    assert wf.keys() == wl.keys() and len(wf) > (100 if kind == "mnv2" else 10)
    assert abs(lf.item() - ll.item()) <= 1e-5 * abs(ll.item())
    w_rel = {k: rel(wf[k], wl[k]) for k in wf}
    hw, hb = w_rel[names[id(last.weight)]], w_rel[names[id(last.bias)]]
    top = max(float(g.norm()) for g in wl.values())
    real = [k for k in wl if float(wl[k].norm()) > 1e-6 * top]
    w_worst_real = max(w_rel[k] for k in real)
    record(kind=kind, yardstick_worst=worst, yardstick_worst_nonzero=worst_real, binary_worst=max(w_rel.values()),
           binary_worst_param=max(w_rel, key=w_rel.get), binary_worst_nonzero=w_worst_real, nonzero_params=len(real),
           params=len(w_rel), head_weight=hw, head_bias=hb)
    print(f"{kind}: yardstick (MobileNetV2UNet(10), plain CE) worst {worst:.3e}, non-zero {worst_real:.3e}; binary "
          f"worst {max(w_rel.values()):.3e}, non-zero ({len(real)} of {len(w_rel)}) {w_worst_real:.3e}, head {hw:.3e} "
          f"{hb:.3e}")
    assert hw < 1e-4 and hb < 1e-4
    assert len(real) > (100 if kind == "mnv2" else 10)
    assert w_worst_real <= 2 * worst_real, (w_worst_real, worst_real)


def test_two_criteria_give_two_plans():
    model = make()
    x, t = batch()
    crits = [BinarySegLoss(dice=1.0, focal_gamma=2.0), BinarySegLoss(dice=0.25, focal_gamma=0.5, pos_weight=3.0),
             BinarySegLoss(dice=1.0, focal_gamma=2.0, threshold=0.3)]  # the threshold is validation's: no new plan
    got, ref = [], []
    with torch.no_grad():
        for c in crits:
            got.append(compute_loss(model, c, x, t).item())
        for c in crits:
            ref.append(c(model(x), t).item())
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-5 * abs(r), (got, ref)
    assert abs(ref[0] - ref[1]) > 1e-3 * abs(ref[0]) and got[0] == got[2]
    keys = [k for k, p in model.__dict__["_segamd_plans"].items() if p.mode == "loss"]
    assert len(keys) == 2  # one plan per set of scalars, the third step reused the first


@pytest.mark.parametrize("kind", KINDS)
def test_bf16io_agrees_with_its_own_logits_path(kind, record):
    """bf16io: the fused loss reads the bf16 low-resolution logits the logits path upsamples, and the kernels' stats
    are bitwise the fp32 entry points' on the same values (tests/test_gpu_binary_loss.py, as tests/test_gpu_bf16io.py
    holds seg_ce_*): the two losses differ by the two blends' rounding alone, 1e-5 as in fp32.  The gradient is the
    fp32 plane, so the head's parameters hold the fp32 figure too."""
    model = make(kind, train=True, conv_math="bf16io")
    x, t = batch()
    last = [m for m in model.modules() if isinstance(m, nn.Conv2d)][-1]
    names = {id(p): k for k, p in model.named_parameters()}
    crit = BinarySegLoss(bce=0.6, dice=1.4, focal_gamma=1.5, pos_weight=2.5, dice_smooth=0.5)
    lf, wf = grads_of(model, lambda: compute_loss(model, crit, x, t))
    ll, wl = grads_of(model, lambda: crit(model(x), t))
    assert torch.isfinite(lf) and abs(lf.item() - ll.item()) <= 1e-5 * abs(ll.item()), (lf.item(), ll.item())
    hw, hb = rel(wf[names[id(last.weight)]], wl[names[id(last.weight)]]), rel(wf[names[id(last.bias)]],
                                                                              wl[names[id(last.bias)]])
    record(kind=kind, loss_fused=lf.item(), loss_logits=ll.item(), head_weight=hw, head_bias=hb)
    print(f"{kind} bf16io: loss {lf.item():.7f} / {ll.item():.7f}, head {hw:.3e} {hb:.3e}")
    assert hw < 1e-4 and hb < 1e-4


@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_validate_fused_equals_unfused(thr, monkeypatch):
    model = make()
    loader = [batch(seed=7), batch(seed=8)]
    head = [m for m in model.modules() if isinstance(m, nn.Conv2d)][-1]
    with torch.no_grad():  # logits on both sides of both thresholds
        head.bias -= model(loader[0][0]).median()
    kw = dict(dice=0.5, pos_weight=2.0, threshold=thr)
    assert fused_loss_options(BinarySegLoss(**kw)) is not None and fused_loss_options(Unfused(**kw)) is None
    copies = []
    orig = torch.Tensor.cpu
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append((self.is_cuda, tuple(self.shape))),
                                                               orig(self, *a, **k))[1])
        r = validate(model, loader, BinarySegLoss(**kw), DEV, progress=False)
    assert engine.bad_label_count(model) is not None
    # one host wait: the 2 x 2 matrix and the three float64 sums come to the host together, and nothing else does
    assert [c for c in copies if c[0]] == [(True, (7,))], copies
    u = validate(model, loader, Unfused(**kw), DEV, progress=False)
    assert tuple(r["confusion"].shape) == (2, 2) == tuple(u["confusion"].shape)
    assert abs(r["loss"] - u["loss"]) <= 1e-5 * abs(u["loss"])
    nvalid = sum(int((t != -100).sum()) for _, t in loader)
    assert int(r["confusion"].sum()) == nvalid == int(u["confusion"].sum())
    zthr = logit_threshold(thr)
    with torch.no_grad():
        close = sum(int((((model(x)[:, 0] - zthr).abs() < MARGIN) & (t != -100)).sum()) for x, t in loader)
    assert close <= MAX_LEFT_OUT * nvalid
    differ = int((r["confusion"] - u["confusion"]).abs().sum()) // 2
    assert differ <= close, (differ, close)
    want = binary_summary(r["confusion"])
    assert all(r[k] == want[k] for k in ("precision", "recall", "f1"))
    assert r["confusion"][:, 1].sum() > 0 and r["confusion"][:, 0].sum() > 0
    # a label of 2 raises at the end of the pass
    x, t = loader[1]
    bad = t.clone()
    bad[1, 9, 9] = 2
    with pytest.raises(IndexError, match="Target out of bounds"):
        validate(model, [loader[0], (x, bad)], BinarySegLoss(**kw), DEV, progress=False)
    with pytest.raises(ValueError):
        validate(model, loader, BinarySegLoss(**kw), DEV, progress=False, tta="hflip")
    with pytest.raises(ValueError):  # binary=True on a model with ten channels
        m10 = deterministic_init(MobileNetV2UNet(10), seed=1).to(DEV).eval()
        m10.forward_loss(x, t, binary=True)


def test_train_one_epoch_lowers_the_loss_and_skips_a_bad_batch():
    model = make(train=True)
    crit = BinarySegLoss(dice=1.0, focal_gamma=1.0, pos_weight=2.0)
    x, t = batch()
    opt = Adam(model.parameters(), lr=1e-3)
    first = train_one_epoch(model, [(x, t)], crit, opt, DEV, progress=False)
    assert engine.bad_label_count(model) is not None
    train_one_epoch(model, [(x, t), (x, t)], crit, opt, DEV, progress=False)
    last = train_one_epoch(model, [(x, t)], crit, opt, DEV, progress=False)
    assert last < first, (first, last)
    steps = {int(st["step"].item()) for st in opt.state.values()}
    assert steps == {4}
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    bad = t.clone()
    bad[1, 5, 5] = 2
    with pytest.raises(IndexError, match="Target out of bounds"):
        train_one_epoch(model, [(x, bad)], crit, opt, DEV, progress=False)
    for k, v in model.named_parameters():
        assert torch.equal(v, before[k]), k  # the step skipped itself on the device
    assert {int(st["step"].item()) for st in opt.state.values()} == {4}


def frame_with_foreground(h, w, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def foreground_model(seed=11):
    """MobileNetV2UNet(1) whose head bias is moved to the frame's median logit: about half the mask is foreground."""
    model = deterministic_init(MobileNetV2UNet(1), seed=seed, random_running_stats=True).to(DEV).eval()
    probe = Predictor(model, frame_hw=(72, 128), target_size=(64, 32), graph=False)
    probe(frame_with_foreground(72, 128))
    head = [m for m in model.modules() if isinstance(m, nn.Conv2d)][-1]
    with torch.no_grad():
        head.bias -= probe.logits().median()
    return model


def test_predictor_threshold(monkeypatch):
    model = foreground_model()
    f = frame_with_foreground(72, 128)
    g = Predictor(model, frame_hw=(72, 128), target_size=(64, 32), threshold=0.5)
    e = Predictor(model, frame_hw=(72, 128), target_size=(64, 32), threshold=0.5, graph=False)
    mg, me = g(f).clone(), e(f).clone()
    assert torch.equal(mg, me) and set(mg.unique().tolist()) == {0, 1}
    # the mask is the thresholded logits, nearest-mapped, away from the margin
    from oracle import cvresize
    z = g.logits()[0, 0].double().cpu().numpy()
    want = cvresize.resize_nearest((z > 0.0).astype(np.uint8), (128, 72))
    close = cvresize.resize_nearest(np.abs(z) < MARGIN, (128, 72))
    assert close.mean() <= MAX_LEFT_OUT
    assert np.array_equal(mg.cpu().numpy()[~close], want[~close])
    # another threshold: fewer foreground pixels
    hi = Predictor(model, frame_hw=(72, 128), target_size=(64, 32), threshold=0.9, graph=False)
    assert 0 <= int(hi(f).sum()) < int(mg.sum())
    # the overlay takes the mask as it is: road = (cls == 1) is the model's foreground
    o = Predictor(model, frame_hw=(72, 128), target_size=(64, 32), threshold=0.5, overlay=True)
    res, det = o.annotate(f)
    assert tuple(res.shape) == (72, 128, 3) and torch.equal(o.mask, mg)
    assert bool(o.overlay.cleaned.any())
    for kw in (dict(temporal=0.5), dict(tta="hflip"), dict(min_confidence=0.5)):
        with pytest.raises(ValueError):
            Predictor(model, frame_hw=(72, 128), target_size=(64, 32), threshold=0.5, graph=False, **kw)
    for thr in (0.0, 1.0, "0.5", True):
        with pytest.raises(ValueError):
            Predictor(model, frame_hw=(72, 128), target_size=(64, 32), threshold=thr, graph=False)
    m10 = deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV).eval()
    with pytest.raises(ValueError):
        Predictor(m10, frame_hw=(72, 128), target_size=(64, 32), threshold=0.5, graph=False)
    # threshold=None: the existing path -- seg_threshold_nearest is never called, and the mask is all 0, as before
    import seg_amd.infer as infer
    called = []
    real_call = infer.call
    monkeypatch.setattr(infer, "call", lambda name, *a: (called.append(name), real_call(name, *a))[1])
    p = Predictor(model, frame_hw=(72, 128), target_size=(64, 32), graph=False)
    assert not bool(p(f).any())
    assert "seg_argmax_nearest" in called and "seg_threshold_nearest" not in called
    called.clear()
    e(f)
    assert "seg_threshold_nearest" in called and "seg_argmax_nearest" not in called
    assert _lib.lib() is not None
