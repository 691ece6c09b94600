"""CPU: seg_amd.OhemCELoss (cross-entropy with online hard example mining) above the kernels -- its torch forward
against an independent BiSeNet-style formulation (`loss[loss > tau]`, else `loss.topk(k)`) on tie-free fp64 inputs,
the tie rule, the special cases, option validation, how the criterion becomes forward_loss / forward_metrics
arguments (seg_amd.train.fused_loss_options), the CPU models' two methods, and the seg_ohem_* launchers' argument
checks, which run before any launch.
"""
import math

import pytest
import torch
from torch import nn
from torch.nn import functional as F

import seg_amd
from seg_amd import OhemCELoss, UNet, _lib, deterministic_init, synthetic_batch, traceable
from seg_amd.build import build
from seg_amd.engine import Ohem, loss_options
from seg_amd.losses import criterion_loss, ohem_loss_terms, resolve_min_kept
from seg_amd.train import compute_loss, fused_loss_options

C = 5
N, H, W = 2, 15, 20
THRESH = 0.7
TAU = -math.log(THRESH)


def _weights():
    return torch.tensor([0.3, 2.0, 0.0, 1.25, 0.7], dtype=torch.float64)


def _case(ignored=True, seed=5):
    """fp64 logits [N, C, H, W] with a margin on the label's logit of about half the pixels (random logits alone leave
    almost every pixel hard, and the top-k branch would never be the one tested), and labels; `ignored`: the first
    three rows of image 0 carry ignore_index."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    y = torch.randint(0, C, (N, H, W), generator=g)
    easy = torch.rand(N, H, W, generator=g) < 0.5
    z.scatter_add_(1, y.unsqueeze(1), (easy * 6.0).unsqueeze(1).to(z.dtype))
    if ignored:
        y[0, :3] = -100
    return z, y


def bisenet(z, y, thresh, k, w=None, ignore_index=-100):
    """BiSeNet's OhemCELoss on the valid pixels, with class weights as a weighted mean over what it keeps."""
    valid = (y != ignore_index).reshape(-1)
    yy = y.reshape(-1)[valid]
    zz = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])[valid]
    loss = F.cross_entropy(zz, yy, reduction="none")
    wy = torch.ones_like(loss) if w is None else w[yy]
    k = min(k, loss.numel())
    hard = loss > -math.log(thresh)
    if int(hard.sum()) >= k:
        idx = hard.nonzero().squeeze(1)
    else:
        idx = loss.topk(k).indices
    return (wy[idx] * loss[idx]).sum() / wy[idx].sum(), idx.numel()


@pytest.mark.parametrize("ignored", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_forward_is_bisenets_formulation(weighted, ignored):
    z, y = _case(ignored)
    w = _weights() if weighted else None
    nv = int((y != -100).sum())
    above = int((ohem_loss_terms(z, y, THRESH, 1)[1]).sum())  # k = 1: threshold mode, K = {l > tau}
    assert 0.25 * nv < above < 0.75 * nv  # about half the pixels are easy
    seen = set()
    for k in (1, above // 2, above + (nv - above) // 2, nv, nv + 50):
        zz = z.clone().requires_grad_(True)
        loss, kept, cut = ohem_loss_terms(zz, y, THRESH, k, w, -100)
        ref, nkept = bisenet(z, y, THRESH, k, w)
        assert abs(loss.item() - ref.item()) <= 1e-13 * abs(ref.item()), (k, loss.item(), ref.item())
        assert int(kept.sum()) == nkept == max(above, min(k, nv))  # tie-free: exactly k in top-k mode
        mode = "threshold" if above >= min(k, nv) else "topk"
        lall = F.cross_entropy(z, y, reduction="none")[y != -100]
        want_cut = TAU if mode == "threshold" else float(lall.sort(descending=True).values[min(k, nv) - 1])
        assert float(cut) == want_cut <= TAU
        assert OhemCELoss(THRESH, k, w)(z, y).item() == loss.item()
        loss.backward()  # the gradient treats K as a constant: exactly 0 outside it
        assert torch.all(zz.grad.permute(0, 2, 3, 1)[~kept] == 0)
        seen.add(mode)
    assert seen == {"threshold", "topk"}


def test_gradient_inside_K_is_the_weighted_softmax_gradient():
    z, y = _case()
    w = _weights()
    k = int((y != -100).sum()) - 40
    zz = z.clone().requires_grad_(True)
    loss, kept, _ = ohem_loss_terms(zz, y, THRESH, k, w)
    loss.backward()
    yy = torch.where(y == -100, torch.zeros_like(y), y)
    onehot = F.one_hot(yy, C).permute(0, 3, 1, 2).to(z.dtype)
    wy = w[yy] * kept
    want = (torch.softmax(z, 1) - onehot) * (wy / wy.sum()).unsqueeze(1)
    assert float((zz.grad - want).abs().max()) < 1e-15
    assert torch.all(zz.grad.permute(0, 2, 3, 1)[~kept] == 0)


def test_a_tie_group_straddling_k_is_kept_whole():
    z, y = _case(ignored=False)
    # nine pixels share one logit vector and label: one loss value, placed in the top-k region
    z[1, :, 4, 2:11] = torch.tensor([0.5, 3.0, 0.125, 0.0, 0.75], dtype=z.dtype).view(C, 1)
    y[1, 4, 2:11] = 1
    l = F.cross_entropy(z, y, reduction="none")
    tie = float(l[1, 4, 2])
    assert torch.all(l[1, 4, 2:11] == tie)
    bigger = int((l > tie).sum())
    above = int((l > TAU).sum())
    assert tie < TAU and bigger >= above  # the group lies below tau: only the floor can keep it
    for k in (bigger + 1, bigger + 4, bigger + 9):
        loss, kept, cut = ohem_loss_terms(z, y, THRESH, k)
        assert int(kept.sum()) == bigger + 9 and bool(kept[1, 4, 2:11].all()) and float(cut) == tie
        assert abs(float(loss) - float(l[kept].mean())) < 1e-14
    assert int(ohem_loss_terms(z, y, THRESH, bigger)[1].sum()) == bigger
    # K does not depend on the pixel order
    perm = torch.randperm(W, generator=torch.Generator().manual_seed(1))
    a = ohem_loss_terms(z, y, THRESH, bigger + 4)[1]
    b = ohem_loss_terms(z[..., perm], y[..., perm], THRESH, bigger + 4)[1]
    assert torch.equal(a[..., perm], b)


def test_special_cases():
    z, y = _case()
    assert torch.isnan(OhemCELoss()(z, torch.full_like(y, -100)))  # 0/0, as aten
    zz = z.clone().requires_grad_(True)
    OhemCELoss()(zz, torch.full_like(y, -100)).backward()
    assert torch.all(zz.grad == 0)
    bad = y.clone()
    bad[1, 2, 3] = C
    with pytest.raises(IndexError):
        OhemCELoss()(z, bad)
    # ignore_index other than the default
    y7 = torch.where(y == -100, torch.full_like(y, 7), y)
    assert float(OhemCELoss(0.7, 100, ignore_index=7)(z, y7)) == float(OhemCELoss(0.7, 100)(z, y))
    # with thresh close to 1 every pixel is hard: plain cross-entropy over the valid pixels
    ce = F.cross_entropy(z, y, ignore_index=-100)
    assert abs(float(OhemCELoss(1 - 1e-12, 1)(z, y)) - float(ce)) < 1e-12
    w = _weights()
    cew = F.cross_entropy(z, y, w, ignore_index=-100)
    assert abs(float(OhemCELoss(1 - 1e-12, 1, weight=w)(z, y)) - float(cew)) < 1e-12


def test_min_kept_as_a_fraction():
    assert resolve_min_kept(17, 1000) == 17
    assert resolve_min_kept(1 / 16, 2 * 15 * 20) == 37  # floor(37.5)
    assert resolve_min_kept(0.001, 600) == 1            # floor(0.6) = 0: at least 1
    assert resolve_min_kept(1.0, 600) == 600
    assert resolve_min_kept(1, 600) == 1                # the int 1 is one pixel, the float 1.0 all of them
    z, y = _case()
    for f in (1 / 16, 0.5, 1.0):
        k = max(1, math.floor(f * N * H * W))
        assert float(OhemCELoss(THRESH, f)(z, y)) == float(OhemCELoss(THRESH, k)(z, y))
    assert OhemCELoss().thresh == 0.7 and OhemCELoss().min_kept == 1 / 16


@pytest.mark.parametrize("kw", [dict(thresh=0.0), dict(thresh=1.0), dict(thresh=-0.1), dict(thresh=1.5),
                                dict(thresh=float("nan")), dict(min_kept=0), dict(min_kept=-3), dict(min_kept=0.0),
                                dict(min_kept=1.5), dict(min_kept=-0.5), dict(min_kept=None), dict(thresh=None)])
def test_option_errors(kw):
    with pytest.raises(ValueError):
        OhemCELoss(**kw)


def test_engine_loss_options():
    dev = torch.device("cpu")
    assert loss_options(None, 0.0, "mean", C, dev) == (None, 0.0, "mean", None)  # the defaults: off
    o = loss_options(None, 0.0, "mean", C, dev, ohem_thresh=0.7, ohem_min_kept=100)
    assert o == (None, 0.0, "mean", Ohem(0.7, 100)) and isinstance(o[3], Ohem)
    assert loss_options(None, 0.0, "mean", C, dev, ohem_thresh=0.5, ohem_min_kept=0.25)[3] == Ohem(0.5, 0.25)
    for bad in (dict(label_smoothing=0.1), dict(reduction="sum"), dict(reduction="none"), dict(dice=0.5),
                dict(focal_gamma=2.0), dict(ce=0.5), dict(ohem_thresh=None), dict(ohem_min_kept=None),
                dict(ohem_thresh=1.0), dict(ohem_min_kept=0), dict(ohem_min_kept=2.0)):
        kw = dict(label_smoothing=0.0, reduction="mean", ohem_thresh=0.7, ohem_min_kept=100)
        kw.update(bad)
        eps, red = kw.pop("label_smoothing"), kw.pop("reduction")
        with pytest.raises(ValueError):
            loss_options(None, eps, red, C, dev, **kw)
        with pytest.raises(ValueError):
            z, y = _case()
            criterion_loss(z, y, label_smoothing=eps, reduction=red, **kw)


def test_fused_loss_options():
    w = _weights().float()
    o = fused_loss_options(OhemCELoss(0.6, 300, weight=w, ignore_index=7))
    assert o["weight"] is not None and torch.equal(o.pop("weight"), w)
    assert o == {"ignore_index": 7, "label_smoothing": 0.0, "reduction": "mean", "ohem_thresh": 0.6,
                 "ohem_min_kept": 300}
    assert fused_loss_options(OhemCELoss())["ohem_min_kept"] == 1 / 16
    assert "ohem_thresh" not in fused_loss_options(nn.CrossEntropyLoss())
    assert "ohem_thresh" not in fused_loss_options(seg_amd.SegLoss(dice=1.0))

    class Scaled(OhemCELoss):
        def forward(self, logits, target):
            return 2 * super().forward(logits, target)

    class Renamed(OhemCELoss):
        pass

    assert fused_loss_options(Scaled()) is None
    assert fused_loss_options(Renamed(0.5, 10))["ohem_min_kept"] == 10


def test_cpu_models_take_the_two_arguments():
    model = deterministic_init(UNet(4, 8), seed=3).eval()
    x, y = synthetic_batch(2, 16, 16, 4, seed=3)
    y[0, :2] = -100
    crit = OhemCELoss(0.7, 0.25, weight=torch.tensor([0.3, 2.0, 0.0, 1.25]))
    with torch.no_grad():
        want = crit(model(x), y)
        for m in (model, traceable(model)):
            got = compute_loss(m, crit, x, y)
            assert float(got) == float(want)
            conf = torch.zeros(4, 4, dtype=torch.int64)
            loss = m.forward_metrics(x, y, conf, **fused_loss_options(crit))
            assert float(loss) == float(want) and int(conf.sum()) == int((y != -100).sum())
    with torch.no_grad():
        plain = model.forward_loss(x, y)  # the defaults: plain cross-entropy
        assert float(plain) == float(F.cross_entropy(model(x), y))
    with pytest.raises(ValueError):
        model.forward_loss(x, y, label_smoothing=0.1, ohem_thresh=0.7, ohem_min_kept=10)
    with pytest.raises(ValueError):
        model.forward_loss(x, y, dice=1.0, ohem_thresh=0.7, ohem_min_kept=10)


def test_launchers_check_their_arguments_before_any_launch():
    build()
    lib = _lib.lib()
    assert _lib.query("seg_ohem_workspace_floats", 1920) >= 1920 + 2048 + 1024 + 1024
    ok = dict(ld=12, C=10, tau=0.35, k=5)
    for bad in (dict(C=0), dict(C=33), dict(ld=10), dict(ld=8), dict(k=0), dict(k=-1), dict(tau=-0.1),
                dict(tau=float("inf")), dict(tau=float("nan"))):
        a = dict(ok, **bad)
        for name in ("seg_ohem_upsample_loss", "seg_ohem_upsample_loss_bf16io"):
            rc = getattr(lib, name)(None, a["ld"], 1, 4, 4, a["C"], None, 8, 8, -100, None, a["tau"], a["k"], None,
                                    None, None)
            assert rc == 1, (name, bad)
        for name in ("seg_ohem_upsample_eval", "seg_ohem_upsample_eval_bf16io"):
            rc = getattr(lib, name)(None, a["ld"], 1, 4, 4, a["C"], None, 8, 8, -100, None, a["tau"], a["k"], None,
                                    None, 1, None)
            assert rc == 1, (name, bad)
        if "k" not in bad:
            assert lib.seg_ohem_upsample_grad(None, a["ld"], 1, 4, 4, a["C"], None, 8, 8, -100, None, a["tau"], None,
                                              None, None, None, 12, None) == 1, bad
            assert lib.seg_ohem_upsample_grad_bf16io(None, a["ld"], 1, 4, 4, a["C"], None, 8, 8, -100, None, a["tau"],
                                                     None, None, None, None, None) == 1, bad  # fp32 NCHW: no ldh
    assert lib.seg_ohem_upsample_eval(None, 12, 1, 4, 4, 10, None, 8, 8, -100, None, 0.35, 5, None, None, None,
                                      None) == 1  # confusion NULL
    assert lib.seg_ohem_upsample_grad(None, 12, 1, 4, 4, 10, None, 8, 8, -100, None, 0.35, None, None, None, None,
                                      10, None) == 1  # ldh % 4
