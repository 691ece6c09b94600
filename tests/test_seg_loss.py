"""CPU: seg_amd.SegLoss (cross-entropy with a focal exponent plus a soft Dice term) above the kernels -- its torch
forward against an independent fp64 evaluation of the definition written with explicit per-class sums in numpy,
nn.CrossEntropyLoss where the two coincide, option validation, how the criterion becomes forward_loss /
forward_metrics arguments (seg_amd.train.fused_loss_options), the CPU models' two methods, and the seg_sl_*
launchers' argument checks, which run before any launch.
"""
import numpy as np
import pytest
import torch
from torch import nn

import seg_amd
from seg_amd import SegLoss, UNet, _lib, deterministic_init, synthetic_batch, traceable
from seg_amd.build import build
from seg_amd.engine import loss_options
from seg_amd.train import compute_loss, fused_loss_options

C = 5
N, H, W = 2, 6, 7


def _weights():
    return torch.tensor([0.3, 2.0, 0.0, 1.25, 0.7], dtype=torch.float64)


def _case(absent=None, all_ignored=False):
    """fp64 logits [N, C, H, W] and labels with the first row of image 0 ignored; `absent`: a class no pixel has."""
    z = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 3
    y = torch.randint(0, C, (N, H, W), generator=torch.Generator().manual_seed(6))
    if absent is not None:
        y[y == absent] = (absent + 1) % C
    y[0, 0] = -100
    if all_ignored:
        y[:] = -100
    return z, y


def numpy_definition(z, y, ce, dice, gamma, w, ignore_index, smooth):
    """The definition of seg_amd/losses.py, pixel by pixel and class by class, in fp64: (loss, F, Dice)."""
    z, y = z.numpy().astype(np.float64), y.numpy()
    Cn = z.shape[1]
    w = np.ones(Cn) if w is None else w.numpy().astype(np.float64)
    num = den = 0.0
    I, S, T = np.zeros(Cn), np.zeros(Cn), np.zeros(Cn)
    for n in range(z.shape[0]):
        for r in range(z.shape[2]):
            for c in range(z.shape[3]):
                lab = int(y[n, r, c])
                if lab == ignore_index:
                    continue
                v = z[n, :, r, c]
                e = np.exp(v - v.max())
                s = e / e.sum()
                pt = s[lab]
                num += w[lab] * (1.0 - pt) ** gamma * -np.log(pt)
                den += w[lab]
                for k in range(Cn):
                    S[k] += s[k]
                I[lab] += s[lab]
                T[lab] += 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.float64(num) / np.float64(den)
    M, dsum = 0, 0.0
    for k in range(Cn):
        if T[k] > 0:
            M += 1
            dsum += 1.0 - (2.0 * I[k] + smooth) / (S[k] + T[k] + smooth)
    D = dsum / max(M, 1)
    loss = (ce * F if ce > 0 else 0.0) + (dice * D if dice > 0 else 0.0)
    return loss, F, D


CASES = [dict(ce=1.0), dict(ce=0.5), dict(ce=0.0, dice=1.0), dict(ce=1.0, focal_gamma=2.0),
         dict(ce=1.0, focal_gamma=0.5), dict(ce=0.7, dice=1.3, focal_gamma=1.5, dice_smooth=0.25)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("absent", [None, 3])
@pytest.mark.parametrize("opts", CASES)
def test_forward_is_the_definition(opts, absent, weighted):
    z, y = _case(absent)
    w = _weights() if weighted else None
    crit = SegLoss(weight=w, **opts)
    got = crit(z, y)
    assert got.dtype == torch.float64
    ref, _, _ = numpy_definition(z, y, crit.ce, crit.dice, crit.focal_gamma, w, -100, crit.dice_smooth)
    assert abs(got.item() - ref) <= 1e-12 * abs(ref), (got.item(), ref)


def test_a_class_absent_from_the_batch_is_left_out_of_the_dice_mean():
    z, y = _case(absent=3)
    _, _, d_absent = numpy_definition(z, y, 0.0, 1.0, 0.0, None, -100, 1.0)
    assert abs(SegLoss(ce=0.0, dice=1.0)(z, y).item() - d_absent) <= 1e-12 * d_absent
    # were the absent class counted (M = C, with its 1 - d_3 = S_3 / (S_3 + smooth) > 0) the mean would differ
    s = torch.softmax(z, 1) * (y != -100).unsqueeze(1)
    S3 = float(s[:, 3].sum())
    counted = (d_absent * (C - 1) + S3 / (S3 + 1.0)) / C
    assert abs(counted - d_absent) > 1e-3 * d_absent


def test_every_pixel_ignored():
    z, y = _case(all_ignored=True)
    assert SegLoss(ce=0.0, dice=1.0)(z, y).item() == 0.0
    assert torch.isnan(SegLoss(ce=1.0)(z, y))
    assert torch.isnan(SegLoss(ce=1.0, focal_gamma=2.0)(z, y))
    assert torch.isnan(SegLoss(ce=1.0, dice=1.0, focal_gamma=2.0)(z, y))
    loss, F, D = numpy_definition(z, y, 1.0, 1.0, 2.0, None, -100, 1.0)
    assert np.isnan(F) and D == 0.0 and np.isnan(loss)


@pytest.mark.parametrize("opts", [dict(), dict(weight=True), dict(label_smoothing=0.1), dict(ignore_index=2),
                                  dict(weight=True, label_smoothing=0.2, ignore_index=1)])
def test_ce_alone_is_cross_entropy(opts):
    opts = dict(opts)
    if opts.pop("weight", False):
        opts["weight"] = _weights()
    z, y = _case()
    y[y == -100] = opts.get("ignore_index", -100)
    z = z.clone().requires_grad_(True)
    a = SegLoss(ce=1.0, **opts)(z, y)
    ga, = torch.autograd.grad(a, z)
    b = nn.CrossEntropyLoss(**opts)(z, y)
    gb, = torch.autograd.grad(b, z)
    assert torch.equal(a, b) and torch.equal(ga, gb)


def test_gradient_is_finite_where_the_label_dominates():
    z, y = _case()
    z = z.float()
    z[1, :, 2, 2] = 0.0
    z[1, int(y[1, 2, 2]), 2, 2] = 200.0  # 1 - pt underflows to exactly 0 in fp32
    z.requires_grad_(True)
    for gamma in (0.5, 2.0):
        loss = SegLoss(ce=1.0, dice=1.0, focal_gamma=gamma)(z, y)
        g, = torch.autograd.grad(loss, z)
        assert torch.isfinite(loss) and torch.isfinite(g).all()


def test_out_of_range_label_raises_index_error():
    z, y = _case()
    y[1, 1, 1] = C
    for opts in (dict(dice=1.0), dict(focal_gamma=2.0)):
        with pytest.raises(IndexError):
            SegLoss(**opts)(z, y)


@pytest.mark.parametrize("bad", [dict(ce=-1.0), dict(dice=-0.5), dict(focal_gamma=-1.0), dict(ce=0.0, dice=0.0),
                                 dict(dice_smooth=0.0), dict(dice_smooth=-1.0), dict(ce=float("nan")),
                                 dict(focal_gamma=float("inf")), dict(label_smoothing=0.1, focal_gamma=2.0),
                                 dict(label_smoothing=1.5)])
def test_option_validation(bad):
    with pytest.raises(ValueError):
        SegLoss(**bad)
    kw = dict(bad)
    eps = kw.pop("label_smoothing", 0.0)
    with pytest.raises(ValueError):
        loss_options(None, eps, "mean", C, torch.device("cpu"), **kw)


def test_engine_loss_options():
    dev = torch.device("cpu")
    assert loss_options(None, 0.0, "mean", C, dev) == (None, 0.0, "mean", None)
    assert loss_options(None, 0.1, "sum", C, dev, dice_smooth=3.0) == (None, 0.1, "sum", None)  # plain CE: no sl
    assert loss_options(None, 0.0, "mean", C, dev, dice=0.5)[3] == (1.0, 0.5, 0.0, 1.0)
    assert loss_options(None, 0.0, "mean", C, dev, 0.5, 0.0, 2, 0.25)[3] == (0.5, 0.0, 2.0, 0.25)
    with pytest.raises(ValueError):
        loss_options(None, 0.0, "sum", C, dev, dice=1.0)  # the mean only
    assert not hasattr(SegLoss(), "reduction")
    assert seg_amd.SegLoss is SegLoss and "SegLoss" in seg_amd.__all__


# ---------------------------------------------------------------- criterion -> options
def test_fused_loss_options():
    w = _weights().float()
    o = fused_loss_options(SegLoss(ce=0.5, dice=2.0, focal_gamma=1.5, weight=w, ignore_index=7, dice_smooth=0.5))
    assert set(o) == {"ignore_index", "weight", "label_smoothing", "reduction", "ce", "dice", "focal_gamma",
                      "dice_smooth"}
    assert torch.equal(o.pop("weight"), w)
    assert o == {"ignore_index": 7, "label_smoothing": 0.0, "reduction": "mean", "ce": 0.5, "dice": 2.0,
                 "focal_gamma": 1.5, "dice_smooth": 0.5}
    assert fused_loss_options(SegLoss(label_smoothing=0.1))["label_smoothing"] == pytest.approx(0.1)
    assert fused_loss_options(nn.CrossEntropyLoss()) == {"ignore_index": -100, "weight": None,
                                                         "label_smoothing": 0.0, "reduction": "mean"}

    class Scaled(SegLoss):
        def forward(self, logits, target):
            return 2 * super().forward(logits, target)

    class Renamed(SegLoss):
        pass

    assert fused_loss_options(Scaled(dice=1.0)) is None
    assert fused_loss_options(Renamed(dice=1.0))["dice"] == 1.0


# ------------------------------------------------------------------------- CPU models
@pytest.fixture(scope="module", params=["model", "traceable"])
def cpu_model(request):
    m = deterministic_init(UNet(4, 8), seed=1).eval()
    return m if request.param == "model" else traceable(m).eval()


@pytest.mark.parametrize("opts", [dict(dice=1.0), dict(focal_gamma=2.0), dict(ce=0.0, dice=1.0),
                                  dict(ce=0.5, dice=1.5, focal_gamma=0.5, dice_smooth=2.0, weight=True)])
def test_cpu_forward_loss_and_metrics_take_the_options(cpu_model, opts):
    opts = dict(opts)
    if opts.pop("weight", False):
        opts["weight"] = torch.tensor([0.3, 2.0, 0.0, 1.25])
    x, y = synthetic_batch(2, 32, 64, 4, seed=3)
    y[0, :2] = -100
    crit = SegLoss(**opts)
    with torch.no_grad():
        logits = cpu_model(x)
        ref = crit(logits, y)
        plain = nn.functional.cross_entropy(logits, y)
        assert not torch.equal(ref, plain)
        assert torch.equal(cpu_model.forward_loss(x, y, **opts), ref)
        assert torch.equal(compute_loss(cpu_model, crit, x, y), ref)
        cm = torch.zeros(4, 4, dtype=torch.int64)
        assert torch.equal(cpu_model.forward_metrics(x, y, cm, **opts), ref)
        cm0 = torch.zeros(4, 4, dtype=torch.int64)
        assert torch.equal(cpu_model.forward_metrics(x, y, cm0), plain)
        assert torch.equal(cpu_model.forward_loss(x, y), plain)  # the defaults: cross-entropy as before
    assert torch.equal(cm, cm0) and int(cm.sum()) == int((y != -100).sum())
    r = seg_amd.validate(cpu_model, [(x, y)], crit, "cpu", progress=False)
    assert r["loss"] == pytest.approx(ref.item(), rel=1e-6) and torch.equal(r["confusion"], cm)


# ---------------------------------------------------------- launcher argument validation
@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.lib()


def test_argument_validation_without_gpu(lib):
    # invalid arguments are rejected before any launch (hipErrorInvalidValue == 1): every buffer is NULL
    ok = dict(ld=12, Cn=10, eps=0.0, ce=1.0, dice=1.0, gamma=2.0, smooth=1.0, ldh=12, conf=8)

    def loss(name, **kw):
        a = {**ok, **kw}
        return getattr(lib, name)(None, a["ld"], 1, 4, 4, a["Cn"], None, 8, 8, -100, None, a["eps"], a["ce"],
                                  a["dice"], a["gamma"], a["smooth"], None, None, None, None)

    def evl(name, **kw):
        a = {**ok, **kw}
        return getattr(lib, name)(None, a["ld"], 1, 4, 4, a["Cn"], None, 8, 8, -100, None, a["eps"], a["ce"],
                                  a["dice"], a["gamma"], a["smooth"], None, None, None, a["conf"], None)

    def grad(name, **kw):
        a = {**ok, **kw}
        return getattr(lib, name)(None, a["ld"], 1, 4, 4, a["Cn"], None, 8, 8, -100, None, a["eps"], a["ce"],
                                  a["dice"], a["gamma"], None, None, None, None, a["ldh"], None)

    nan = float("nan")
    for sfx in ("", "_bf16io"):
        for fn, name in ((loss, "seg_sl_upsample_loss"), (evl, "seg_sl_upsample_eval"),
                         (grad, "seg_sl_upsample_grad")):
            name += sfx
            assert fn(name, gamma=-0.5) == 1 and fn(name, gamma=nan) == 1 and fn(name, gamma=float("inf")) == 1
            assert fn(name, ce=-1.0) == 1 and fn(name, dice=-1.0) == 1 and fn(name, ce=nan) == 1
            assert fn(name, ce=0.0, dice=0.0) == 1                      # both coefficients zero
            assert fn(name, eps=-0.1) == 1 and fn(name, eps=1.5) == 1
            assert fn(name, eps=0.1) == 1                               # smoothing with gamma > 0
            assert fn(name, Cn=33, ld=36, ldh=36) == 1 and fn(name, Cn=0) == 1
            assert fn(name, ld=10) == 1 and fn(name, ld=8) == 1         # ld % 4 != 0, ld < C
        for fn, name in ((loss, "seg_sl_upsample_loss"), (evl, "seg_sl_upsample_eval")):
            assert fn(name + sfx, smooth=0.0) == 1 and fn(name + sfx, smooth=-1.0) == 1
        assert evl("seg_sl_upsample_eval" + sfx, conf=None) == 1        # NULL confusion
        assert grad("seg_sl_upsample_grad" + sfx, ldh=10) == 1 and grad("seg_sl_upsample_grad" + sfx, ldh=8) == 1
    per_block = 6 + 3 * 32
    assert _lib.query("seg_sl_workspace_floats", 1) == per_block
    assert _lib.query("seg_sl_workspace_floats", 4 * 256 * 512) == 2048 * per_block
