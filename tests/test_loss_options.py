"""CPU: the fused loss's options (class weights, label smoothing, reduction "sum") above the
kernels -- how a criterion becomes forward_loss / forward_metrics arguments
(seg_amd.train.fused_loss_options), the torch composition of both methods on CPU tensors,
seg_amd.class_weights, and the seg_cew_* launchers' argument checks, which run before any launch.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import seg_amd
from seg_amd import UNet, _lib, class_weights, deterministic_init, synthetic_batch, traceable
from seg_amd.build import build
from seg_amd.train import compute_loss, fused_loss_options

C = 4


def _weights():
    return torch.tensor([0.3, 2.0, 0.0, 1.25])


# ---------------------------------------------------------------- criterion -> options
def test_plain_criterion_gives_the_defaults():
    assert fused_loss_options(nn.CrossEntropyLoss()) == {"ignore_index": -100, "weight": None,
                                                         "label_smoothing": 0.0, "reduction": "mean"}


def test_weight_smoothing_sum_and_ignore_index_are_picked_up():
    w = _weights()
    o = fused_loss_options(nn.CrossEntropyLoss(weight=w, label_smoothing=0.1, reduction="sum", ignore_index=7))
    assert o["weight"] is not None and torch.equal(o["weight"], w)
    assert o["label_smoothing"] == pytest.approx(0.1) and o["reduction"] == "sum" and o["ignore_index"] == 7


def test_criteria_that_keep_the_logits_path():
    class Scaled(nn.CrossEntropyLoss):
        def forward(self, input, target):
            return 2 * super().forward(input, target)

    class Renamed(nn.CrossEntropyLoss):  # no forward of its own: still the aten loss
        pass

    assert fused_loss_options(nn.CrossEntropyLoss(reduction="none")) is None
    assert fused_loss_options(Scaled()) is None
    assert fused_loss_options(nn.NLLLoss()) is None
    assert fused_loss_options(lambda a, b: a.sum()) is None
    assert fused_loss_options(Renamed(label_smoothing=0.2))["label_smoothing"] == pytest.approx(0.2)


# ------------------------------------------------------------------------- CPU models
def _batch():
    x, y = synthetic_batch(2, 32, 64, C, seed=3)
    y[0, :2] = -100
    return x, y


@pytest.fixture(scope="module", params=["model", "traceable"])
def cpu_model(request):
    m = deterministic_init(UNet(C, 8), seed=1).eval()
    return m if request.param == "model" else traceable(m).eval()


@pytest.mark.parametrize("opts", [dict(weight=True), dict(label_smoothing=0.1), dict(reduction="sum"),
                                  dict(weight=True, label_smoothing=0.1, reduction="sum")])
def test_cpu_forward_loss_and_metrics_take_the_options(cpu_model, opts):
    opts = dict(opts)
    if opts.pop("weight", False):
        opts["weight"] = _weights()
    x, y = _batch()
    with torch.no_grad():
        logits = cpu_model(x)
        ref = F.cross_entropy(logits, y, **opts)
        plain = F.cross_entropy(logits, y)
        assert not torch.equal(ref, plain)  # the options matter on this batch
        assert torch.equal(cpu_model.forward_loss(x, y, **opts), ref)
        cm = torch.zeros(C, C, dtype=torch.int64)
        assert torch.equal(cpu_model.forward_metrics(x, y, cm, **opts), ref)
        cm0 = torch.zeros(C, C, dtype=torch.int64)
        assert torch.equal(cpu_model.forward_metrics(x, y, cm0), plain)
    assert torch.equal(cm, cm0) and int(cm.sum()) == int((y != -100).sum())


def test_compute_loss_and_validate_pass_the_criterion_on():
    model = deterministic_init(UNet(C, 8), seed=1).eval()
    crit = nn.CrossEntropyLoss(weight=_weights(), label_smoothing=0.1)
    x, y = _batch()
    calls = []
    real = model.forward_loss
    model.forward_loss = lambda *a, **k: calls.append(k) or real(*a, **k)
    with torch.no_grad():
        assert torch.equal(compute_loss(model, crit, x, y), crit(model(x), y))
    assert len(calls) == 1 and calls[0]["label_smoothing"] == pytest.approx(0.1)
    del model.forward_loss
    r = seg_amd.validate(model, [(x, y)], crit, "cpu", progress=False)
    r0 = seg_amd.validate(model, [(x, y)], nn.CrossEntropyLoss(), "cpu", progress=False)
    with torch.no_grad():
        assert r["loss"] == pytest.approx(crit(model(x), y).item(), rel=1e-6)
    assert r["loss"] != r0["loss"] and torch.equal(r["confusion"], r0["confusion"])


# ---------------------------------------------------------------------- class_weights
def test_class_weights_vector_and_matrix_agree():
    counts = torch.tensor([900, 40, 0, 10, 50])
    cm = torch.tensor([[800, 100, 0, 0, 0],
                       [10, 20, 5, 5, 0],
                       [0, 0, 0, 0, 0],
                       [1, 2, 3, 4, 0],
                       [0, 0, 0, 25, 25]])
    assert torch.equal(cm.sum(1), counts)
    for scheme in ("median_frequency", "inverse"):
        w = class_weights(counts, scheme)
        assert w.dtype == torch.float32 and tuple(w.shape) == (5,)
        assert torch.equal(w, class_weights(cm, scheme))
        assert torch.equal(w, class_weights(counts.tolist(), scheme))
        assert w[2].item() == 0.0 and bool((w[[0, 1, 3, 4]] > 0).all())


def test_class_weights_schemes_and_clip():
    counts = torch.tensor([900, 40, 0, 10, 50])
    w = class_weights(counts)  # present counts 10, 40, 50, 900: the (lower) median is 40
    assert w[1].item() == 1.0
    assert w.tolist() == pytest.approx([40 / 900, 1.0, 0.0, 4.0, 0.8], rel=1e-6)
    assert class_weights(torch.tensor([5, 1, 9]))[0].item() == 1.0  # odd number of classes: the middle one
    wi = class_weights(counts, "inverse")
    assert wi.tolist() == pytest.approx([1000 / (4 * n) if n else 0.0 for n in counts.tolist()], rel=1e-6)
    assert float((wi.double() * counts).sum()) == pytest.approx(1000.0, rel=1e-6)  # mean weight per pixel = 1
    wc = class_weights(counts, clip=2.0)
    assert wc[3].item() == 2.0 and torch.equal(wc[[0, 1, 2, 4]], w[[0, 1, 2, 4]])
    assert class_weights(torch.zeros(3)).tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        class_weights(counts, "balanced")
    with pytest.raises(ValueError):
        class_weights(torch.zeros(2, 3))
    assert seg_amd.class_weights is class_weights and "class_weights" in seg_amd.__all__


# ---------------------------------------------------------- launcher argument validation
@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.lib()


def test_argument_validation_without_gpu(lib):
    # invalid arguments are rejected before any launch (hipErrorInvalidValue == 1): every buffer is NULL
    def loss(name, ld=12, Cn=10, eps=0.1, red=0):
        return getattr(lib, name)(None, ld, 1, 4, 4, Cn, None, 8, 8, -100, None, eps, red, None, None, None)

    def evl(name, ld=12, Cn=10, eps=0.1, red=0, conf=8):
        return getattr(lib, name)(None, ld, 1, 4, 4, Cn, None, 8, 8, -100, None, eps, red, None, None, conf, None)

    def grad(name, ld=12, Cn=10, eps=0.1, ldh=12):
        return getattr(lib, name)(None, ld, 1, 4, 4, Cn, None, 8, 8, -100, None, eps, None, None, None, ldh, None)

    for sfx in ("", "_bf16io"):
        for fn, name in ((loss, "seg_cew_upsample_loss"), (evl, "seg_cew_upsample_eval")):
            name += sfx
            assert fn(name, red=2) == 1 and fn(name, red=-1) == 1  # unknown reduction
            assert fn(name, eps=-0.1) == 1 and fn(name, eps=1.5) == 1 and fn(name, eps=float("nan")) == 1
            assert fn(name, ld=10) == 1   # ld % 4 != 0
            assert fn(name, Cn=33, ld=36) == 1 and fn(name, Cn=0) == 1
        assert evl("seg_cew_upsample_eval" + sfx, conf=None) == 1  # NULL confusion
        g = "seg_cew_upsample_grad" + sfx
        assert grad(g, eps=-0.1) == 1 and grad(g, eps=1.5) == 1
        assert grad(g, ld=10) == 1 and grad(g, ldh=10) == 1 and grad(g, Cn=33, ld=36, ldh=36) == 1
    assert _lib.query("seg_cew_workspace_floats", 4 * 256 * 512) >= 5
    assert _lib.query("seg_cew_workspace_floats", 1) == 5


def test_every_family_checks_its_geometry_before_any_launch(lib):
    # one table of bad geometries for seg_ce_*, seg_cew_*, seg_sl_* and seg_kd_* (seg_ohem_*: tests/test_ohem_loss.py):
    # every entry point returns hipErrorInvalidValue (1) with every buffer NULL, so nothing was launched.  The options
    # are valid ones and the teacher / confusion pointers non-NULL (never read): the geometry is what is refused.
    head = lambda a: (None, a["ld"], 1, 4, 4, a["C"])
    lab = (None, 8, 8, -100)
    te = (16, 12, 4, 4)  # teacher rows, ldt, Ht, Wt
    fams = {
        "seg_ce": dict(fwd=lambda a: head(a) + lab + (None, None), grad=lambda a: head(a) + lab),
        "seg_cew": dict(fwd=lambda a: head(a) + lab + (None, 0.1, 0, None, None),
                        grad=lambda a: head(a) + lab + (None, 0.1)),
        "seg_sl": dict(fwd=lambda a: head(a) + lab + (None, 0.0, 1.0, 0.5, 0.0, 1.0, None, None, None),
                       grad=lambda a: head(a) + lab + (None, 0.0, 1.0, 0.5, 0.0), table=(None,)),
        "seg_kd": dict(fwd=lambda a: head(a) + te + lab + (None, 1.0, 0.5, 2.0, 1, None, None),
                       grad=lambda a: head(a) + te + lab + (None, 1.0, 0.5, 2.0, 1), eval=False),
    }
    ok = dict(ld=12, C=10, ldh=12, conf=8)
    table = (dict(C=0), dict(C=33, ld=36, ldh=36), dict(ld=10), dict(ld=8), dict(ldh=10), dict(ldh=8), dict(conf=None))
    for stem, fam in fams.items():
        for bad in table:
            a = dict(ok, **bad)
            for sfx in ("", "_bf16io"):
                if "ldh" not in bad or "C" in bad:
                    if "conf" not in bad:
                        assert getattr(lib, f"{stem}_upsample_loss{sfx}")(*fam["fwd"](a), None) == 1, (stem, sfx, bad)
                    if fam.get("eval", True):
                        assert getattr(lib, f"{stem}_upsample_eval{sfx}")(*fam["fwd"](a), a["conf"], None) == 1, \
                            (stem, sfx, bad)
                if "conf" not in bad:
                    args = fam["grad"](a) + (None, None) + fam.get("table", ()) + (None,)
                    assert getattr(lib, f"{stem}_upsample_grad{sfx}")(*args, a["ldh"], None) == 1, (stem, sfx, bad)
            if stem == "seg_kd" and "ldh" not in bad and "conf" not in bad:  # the fp32 NCHW twin has no ldh
                args = fam["grad"](a) + (None, None, None)
                assert lib.seg_kd_upsample_grad_bf16io_nchw(*args, None) == 1, bad
