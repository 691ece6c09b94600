"""CPU: seg_amd.DistillLoss (pixel-wise knowledge distillation) above the kernels -- distill_loss_terms in fp64 against
an independent formula (F.cross_entropy + T^2 F.kl_div), its autograd gradient against the closed form, the special
cases, option validation, that the teacher is no part of the criterion's state, how the criterion becomes forward_loss
arguments (seg_amd.train.fused_loss_options), one training epoch and one validation pass on CPU models, and the
seg_kd_* / seg_low_logits_f32 launchers' argument checks, which run before any launch.
"""
import math

import pytest
import torch
from torch import nn
from torch.nn import functional as F

import seg_amd
from seg_amd import DistillLoss, MobileNetV2UNet, UNet, _lib, deterministic_init, synthetic_batch
from seg_amd.build import build
from seg_amd.engine import Distill, loss_options
from seg_amd.losses import check_distill_options, distill_loss_terms
from seg_amd.train import compute_loss, fused_loss_options, train_one_epoch, validate

C = 5
N, H, W = 2, 15, 20


def _weights():
    return torch.tensor([0.3, 2.0, 0.0, 1.25, 0.7], dtype=torch.float64)


def _case(ignored=True, seed=5):
    """fp64 student and teacher logits [N, C, H, W] (independent) and labels; the first three rows of image 0 carry
    ignore_index."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    u = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2
    y = torch.randint(0, C, (N, H, W), generator=g)
    if ignored:
        y[0, :3] = -100
    return z, u, y


def independent(z, u, y, ce, kd, T, w, kd_ignored):
    """ce F.cross_entropy + kd T^2 F.kl_div(log_softmax(z / T), softmax(u / T), "sum") / |P| over the pixels of P."""
    zr = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    ur = u.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    keep = torch.ones_like(y.reshape(-1), dtype=torch.bool) if kd_ignored else (y.reshape(-1) != -100)
    KD = T * T * F.kl_div(F.log_softmax(zr[keep] / T, 1), F.softmax(ur[keep] / T, 1), reduction="sum") / int(keep.sum())
    CE = F.cross_entropy(z, y, w, ignore_index=-100)
    return (ce * CE if ce > 0 else 0.0) + kd * KD, CE, KD


@pytest.mark.parametrize("kd_ignored", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ce,kd,T", [(1.0, 1.0, 2.0), (0.0, 0.7, 4.0), (0.5, 2.0, 1.0)])
def test_terms_against_the_independent_formula(ce, kd, T, weighted, kd_ignored):
    z, u, y = _case()
    w = _weights() if weighted else None
    loss, CE, KD = distill_loss_terms(z, u, y, ce, kd, T, w, -100, kd_ignored)
    want, wCE, wKD = independent(z, u, y, ce, kd, T, w, kd_ignored)
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
    assert abs(float(KD) - float(wKD)) <= 1e-12 * abs(float(wKD)) and 0.5 < float(KD) < 4.0
    if ce > 0:
        assert abs(float(CE) - float(wCE)) <= 1e-12 * abs(float(wCE))
    else:
        assert CE is None
    assert float(DistillLoss(nn.Identity(), ce, kd, T, w, kd_ignored=kd_ignored)(z, y, u)) == float(loss)


@pytest.mark.parametrize("kd_ignored", [True, False])
@pytest.mark.parametrize("ce", [1.0, 0.0])
def test_gradient_is_the_closed_form(ce, kd_ignored):
    z, u, y = _case()
    w, kd, T, g = _weights(), 0.8, 2.0, 0.7
    zr = z.clone().requires_grad_(True)
    ur = u.clone().requires_grad_(True)
    loss = distill_loss_terms(zr, ur, y, ce, kd, T, w, -100, kd_ignored)[0]
    loss.backward(torch.tensor(g, dtype=torch.float64))
    assert ur.grad is None  # the teacher gets no gradient
    valid = (y != -100)
    yy = torch.where(valid, y, torch.zeros_like(y))
    D = float(w[yy][valid].sum())
    P = y.numel() if kd_ignored else int(valid.sum())
    onehot = F.one_hot(yy, C).permute(0, 3, 1, 2).double()
    hard = (ce / D) * w[yy].unsqueeze(1) * (torch.softmax(z, 1) - onehot) * valid.unsqueeze(1)
    inP = torch.ones_like(valid) if kd_ignored else valid
    soft = kd * T / P * (torch.softmax(z / T, 1) - torch.softmax(u / T, 1)) * inP.unsqueeze(1)
    want = g * (hard + soft)
    assert float((zr.grad - want).abs().max()) <= 1e-14
    if not kd_ignored:
        assert not zr.grad[0, :, :3].any()  # outside P and V: exactly 0


def test_kd_is_zero_for_the_student_itself_and_ignores_a_per_pixel_constant():
    z, u, y = _case()
    for T in (1.0, 2.0, 4.0):
        assert float(distill_loss_terms(z, z.clone(), y, 0.0, 1.0, T)[2]) == 0.0
        a = distill_loss_terms(z, u, y, 0.0, 1.0, T)[2]
        shift = torch.randn(N, 1, H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 5
        b = distill_loss_terms(z, u + shift, y, 0.0, 1.0, T)[2]
        assert abs(float(a) - float(b)) <= 1e-12 * float(a)


def test_no_valid_pixel():
    z, u, y = _case()
    y = torch.full_like(y, -100)
    assert math.isfinite(float(distill_loss_terms(z, u, y, 0.0, 1.0, 2.0)[0]))        # ce = 0: the CE's 0/0 left out
    assert math.isnan(float(distill_loss_terms(z, u, y, 1.0, 1.0, 2.0)[0]))           # as nn.CrossEntropyLoss
    assert math.isnan(float(distill_loss_terms(z, u, y, 0.0, 1.0, 2.0, kd_ignored=False)[0]))  # P empty
    y[0, 0, 0] = C
    with pytest.raises(IndexError):
        distill_loss_terms(z, u, y)


@pytest.mark.parametrize("kw", [dict(kd=0.0), dict(kd=-1.0), dict(kd=float("nan")), dict(kd=float("inf")),
                                dict(ce=-0.1), dict(ce=float("inf")), dict(ce=float("nan")),
                                dict(temperature=0.0), dict(temperature=-2.0), dict(temperature=float("inf")),
                                dict(temperature=float("nan"))])
def test_refused_options(kw):
    with pytest.raises(ValueError):
        DistillLoss(nn.Identity(), **kw)
    a = dict(ce=1.0, kd=1.0, temperature=2.0)
    a.update(kw)
    with pytest.raises(ValueError):
        check_distill_options(a["ce"], a["kd"], a["temperature"])
    if a["kd"] != 0.0:  # kd = 0 is forward_loss's default: no distillation asked for
        with pytest.raises(ValueError):
            loss_options(None, 0.0, "mean", C, torch.device("cpu"), ce=a["ce"], kd=a["kd"],
                         kd_temperature=a["temperature"])


@pytest.mark.parametrize("kw", [dict(label_smoothing=0.1), dict(reduction="sum"), dict(reduction="none"),
                                dict(dice=1.0), dict(focal_gamma=2.0), dict(ohem_thresh=0.7, ohem_min_kept=10)])
def test_not_combined_with_the_other_families(kw):
    a = dict(weight=None, label_smoothing=0.0, reduction="mean", C=C, device=torch.device("cpu"), kd=1.0,
             kd_temperature=2.0)
    a.update(kw)
    with pytest.raises(ValueError):
        loss_options(**a)
    ok = loss_options(None, 0.0, "mean", C, torch.device("cpu"), ce=0.0, kd=1.5, kd_temperature=4.0, kd_ignored=False)
    assert ok == (None, 0.0, "mean", Distill(0.0, 1.5, 4.0, False, 0, 0))
    # the defaults: what they always gave
    assert loss_options(None, 0.0, "mean", C, torch.device("cpu")) == (None, 0.0, "mean", None)


def _teacher_student():
    teacher = deterministic_init(UNet(10, 8), seed=3)
    student = deterministic_init(MobileNetV2UNet(10), seed=4)
    return teacher, student


def test_the_teacher_is_no_part_of_the_criterion():
    teacher = deterministic_init(UNet(10, 8), seed=3).train()
    for p in teacher.parameters():
        assert p.requires_grad
    w = torch.rand(10)
    crit = DistillLoss(teacher, weight=w)
    assert not teacher.training and all(not p.requires_grad for p in teacher.parameters())
    assert list(crit.parameters()) == [] and list(crit.children()) == []
    assert list(crit.state_dict()) == ["weight"] and crit.teacher is teacher
    assert [k for k, _ in crit.named_buffers()] == ["weight"]
    crit.double()  # the criterion's own bookkeeping leaves the teacher alone
    assert crit.weight.dtype == torch.float64 and next(teacher.parameters()).dtype == torch.float32
    assert isinstance(crit.hard(), nn.CrossEntropyLoss) and crit.hard().ignore_index == -100
    assert torch.equal(crit.hard().weight, crit.weight)
    x, y = synthetic_batch(1, 32, 32, 10, seed=3)
    tl = crit.teacher_logits(x)
    assert tuple(tl.shape) == (1, 10, 32, 32) and not tl.requires_grad
    teacher.train()
    with pytest.raises(RuntimeError):
        crit.teacher_logits(x)
    with pytest.raises(RuntimeError):
        crit(tl, y, tl)
    with pytest.raises(TypeError):
        DistillLoss(lambda x: x)


def test_fused_loss_options_of_a_distill_loss():
    w = torch.rand(10)
    o = fused_loss_options(DistillLoss(nn.Identity(), 0.5, 2.0, 4.0, weight=w, ignore_index=7, kd_ignored=False))
    assert torch.equal(o.pop("weight"), w)
    assert o == {"ignore_index": 7, "label_smoothing": 0.0, "reduction": "mean", "ce": 0.5, "kd": 2.0,
                 "kd_temperature": 4.0, "kd_ignored": False}
    d = fused_loss_options(DistillLoss(nn.Identity()))
    assert (d["ce"], d["kd"], d["kd_temperature"], d["kd_ignored"], d["weight"]) == (1.0, 1.0, 2.0, True, None)
    assert "kd" not in fused_loss_options(nn.CrossEntropyLoss())
    assert "kd" not in fused_loss_options(seg_amd.SegLoss(dice=1.0))
    assert "kd" not in fused_loss_options(seg_amd.OhemCELoss())

    class Scaled(DistillLoss):
        def forward(self, logits, target, teacher_logits):
            return 2 * super().forward(logits, target, teacher_logits)

    class Renamed(DistillLoss):
        pass

    assert fused_loss_options(Scaled(nn.Identity())) is None
    assert fused_loss_options(Renamed(nn.Identity(), kd=3.0))["kd"] == 3.0


def test_one_epoch_and_validation_on_cpu_models():
    teacher, student = _teacher_student()
    crit = DistillLoss(teacher, ce=1.0, kd=1.0, temperature=2.0)
    x, y = synthetic_batch(2, 64, 64, 10, seed=7)
    y[0, :3] = -100
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    assert any("running_mean" in k for k in before) and any("num_batches_tracked" in k for k in before)
    student.train()
    with torch.no_grad():
        want = crit(student(x), y, crit.teacher_logits(x))
    student = deterministic_init(MobileNetV2UNet(10), seed=4).train()  # the forward above moved its BN statistics
    opt = torch.optim.SGD(student.parameters(), lr=0.0)
    got = train_one_epoch(student, [(x, y)], crit, opt, "cpu", progress=False)
    assert abs(got - float(want)) <= 1e-6 * abs(float(want))
    after = teacher.state_dict()
    assert before.keys() == after.keys()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert not teacher.training and all(p.grad is None for p in teacher.parameters())
    grads = [p.grad for p in student.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(torch.isfinite(g).all() for g in grads) and any(g.any() for g in grads)
    with pytest.raises(RuntimeError):  # GPU only, as the models' own forward
        student.forward_loss(x, y, kd=1.0, teacher_logits=torch.zeros(2, 32, 32, 12))
    with pytest.raises(RuntimeError):
        teacher.forward_low_logits(x)
    # validation does not distil: hard()'s loss, the plain criterion's matrix
    r = validate(student, [(x, y)], crit, "cpu", progress=False)
    r0 = validate(student, [(x, y)], crit.hard(), "cpu", progress=False)
    student.eval()
    with torch.no_grad():
        ref = float(crit.hard()(student(x), y))
    assert r["loss"] == r0["loss"] and abs(r["loss"] - ref) <= 1e-6 * abs(ref)
    assert torch.equal(r["confusion"], r0["confusion"])
    assert not teacher.training


def test_compute_loss_on_the_cpu_is_the_unfused_form():
    teacher, student = _teacher_student()
    student.eval()
    crit = DistillLoss(teacher, kd_ignored=False, weight=torch.rand(10, generator=torch.Generator().manual_seed(2)))
    x, y = synthetic_batch(1, 32, 32, 10, seed=5)
    with torch.no_grad():
        assert float(compute_loss(student, crit, x, y)) == float(crit(student(x), y, teacher(x)))


def _kd_loss(lib, name, ld=12, C=10, teacher=64, ldt=12, Ht=4, Wt=4, ce=1.0, kd=1.0, T=2.0):
    return getattr(lib, name)(None, ld, 1, 4, 4, C, teacher, ldt, Ht, Wt, None, 8, 8, -100, None, ce, kd, T, 1, None,
                              None, None)


def _kd_grad(lib, name, ld=12, C=10, teacher=64, ldt=12, Ht=4, Wt=4, ce=1.0, kd=1.0, T=2.0, ldh=12):
    args = [None, ld, 1, 4, 4, C, teacher, ldt, Ht, Wt, None, 8, 8, -100, None, ce, kd, T, 1, None, None, None]
    if not name.endswith("_nchw"):
        args.append(ldh)
    return getattr(lib, name)(*args, None)


def test_launchers_check_their_arguments_before_any_launch():
    build()
    lib = _lib.lib()
    inf, nan = float("inf"), float("nan")
    bads = [dict(C=0), dict(C=33), dict(ld=10), dict(ld=8), dict(ldt=10), dict(ldt=8), dict(Ht=0), dict(Wt=0),
            dict(Ht=-1), dict(kd=0.0), dict(kd=-1.0), dict(kd=inf), dict(kd=nan), dict(ce=-0.5), dict(ce=inf),
            dict(ce=nan), dict(T=0.0), dict(T=-1.0), dict(T=inf), dict(T=nan), dict(teacher=None)]
    for bad in bads:
        for name in ("seg_kd_upsample_loss", "seg_kd_upsample_loss_bf16io"):
            assert _kd_loss(lib, name, **bad) == 1, (name, bad)
        for name in ("seg_kd_upsample_grad", "seg_kd_upsample_grad_bf16io", "seg_kd_upsample_grad_bf16io_nchw"):
            assert _kd_grad(lib, name, **bad) == 1, (name, bad)
    for name in ("seg_kd_upsample_grad", "seg_kd_upsample_grad_bf16io"):
        assert _kd_grad(lib, name, ldh=10) == 1 and _kd_grad(lib, name, ldh=8) == 1, name
    for name in ("seg_low_logits_f32", "seg_low_logits_f32_bf16io"):
        fn = getattr(lib, name)
        assert fn(64, 10, 4, 10, 64, 12, None) == 1    # ld % 4
        assert fn(64, 8, 4, 10, 64, 12, None) == 1     # ld < C
        assert fn(64, 12, 4, 10, 64, 10, None) == 1    # ldo % 4
        assert fn(64, 12, 4, 10, 64, 8, None) == 1     # ldo < C
        assert fn(64, 12, 4, 0, 64, 12, None) == 1     # C < 1
        assert fn(None, 12, 4, 10, 64, 12, None) == 1 and fn(64, 12, 4, 10, None, 12, None) == 1


def test_workspace_query():
    build()
    sizes = [_lib.query("seg_kd_workspace_floats", p) for p in (1, 255, 257, 1920, 1 << 16, 1 << 19, 1 << 22)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
