"""CPU: seg_amd.BinarySegLoss -- the definition in torch ops (the reference the seg_bce_* kernels are tested against),
its option checks, how train.py recognises it, validate() on a one-logit model, and the C ABI's declarations."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import seg_amd
from seg_amd import BinarySegLoss, LightUNet, deterministic_init
from seg_amd.engine import loss_options
from seg_amd.losses import binary_loss_terms, logit_threshold
from seg_amd.metrics import binary_summary
from seg_amd.train import fused_loss_options, validate

from test_abi import CTYPE, header_decls


def data(N=2, H=6, W=7, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(N, 1, H, W, generator=g) * 2).to(dtype)
    t = torch.randint(0, 2, (N, H, W), generator=g)
    return z, t


@pytest.mark.parametrize("pos_weight", [1.0, 2.5, 0.3])
def test_gamma0_is_bce_with_logits(pos_weight):
    z, t = data()
    got = BinarySegLoss(pos_weight=pos_weight)(z, t)
    ref = F.binary_cross_entropy_with_logits(z[:, 0], t.double(), pos_weight=torch.tensor(pos_weight,
                                                                                          dtype=torch.float64))
    assert abs(float(got) - float(ref)) <= 1e-12
    same = nn.BCEWithLogitsLoss(pos_weight=torch.tensor(pos_weight))(z[:, 0].float(), t.float())
    assert abs(float(got) - float(same)) <= 1e-6


def test_terms_follow_the_definition():
    """F, Dice and their sum, written out pixel by pixel in Python floats."""
    z, t = data(1, 3, 4, seed=3)
    t[0, 0, :2] = -100
    bce, dice, gamma, pw, smooth = 0.6, 1.4, 1.5, 2.5, 0.5
    f = I = S = T = 0.0
    n = 0
    for zp, tp in zip(z.reshape(-1).tolist(), t.reshape(-1).tolist()):
        if tp == -100:
            continue
        s = 1.0 / (1.0 + math.exp(-zp))
        pt = s if tp == 1 else 1.0 - s
        f += (pw if tp == 1 else 1.0) * (1.0 - pt) ** gamma * -math.log(pt)
        I, S, T, n = I + s * tp, S + s, T + tp, n + 1
    want_f, want_d = f / n, 1.0 - (2.0 * I + smooth) / (S + T + smooth)
    loss, focal, soft = binary_loss_terms(z, t, bce, dice, gamma, pw, -100, smooth)
    assert abs(float(focal) - want_f) < 1e-12 and abs(float(soft) - want_d) < 1e-12
    assert abs(float(loss) - (bce * want_f + dice * want_d)) < 1e-12
    assert binary_loss_terms(z, t, 1.0, 0.0)[2] is None and binary_loss_terms(z, t, 0.0, 1.0)[1] is None


@pytest.mark.parametrize("opts", [dict(), dict(focal_gamma=0.5), dict(dice=1.0, focal_gamma=2.0, pos_weight=2.5),
                                  dict(bce=0.0, dice=1.0)])
def test_gradient_is_exactly_zero_on_ignored_pixels(opts):
    z, t = data()
    t[0, :2] = -100
    z.requires_grad_(True)
    BinarySegLoss(**opts)(z, t).backward()
    assert torch.all(z.grad[0, 0, :2] == 0) and torch.isfinite(z.grad).all()
    assert float(z.grad[0, 0, 2:].abs().min()) > 0


def test_no_valid_pixel():
    z, t = data()
    t[:] = -100
    assert torch.isnan(BinarySegLoss()(z, t))
    assert torch.isnan(BinarySegLoss(dice=1.0)(z, t))
    only_dice = BinarySegLoss(bce=0, dice=1)(z, t)  # the term whose coefficient is 0 is left out, its NaN included
    assert torch.isfinite(only_dice) and float(only_dice) == 0.0


def test_out_of_range_label_and_float_target():
    z, t = data()
    for bad in (2, -1, 255):
        u = t.clone()
        u[1, 2, 3] = bad
        with pytest.raises(IndexError):
            BinarySegLoss()(z, u)
    with pytest.raises(TypeError):
        BinarySegLoss()(z, t.double())
    with pytest.raises(TypeError):
        BinarySegLoss()(z, t.float().unsqueeze(1))
    with pytest.raises(ValueError):
        BinarySegLoss()(torch.cat([z, z], 1), t)  # two channels


def test_target_shapes_and_dtypes():
    z, t = data()
    crit = BinarySegLoss(dice=0.5, focal_gamma=1.0, pos_weight=2.0)
    want = crit(z, t)
    for u in (t.unsqueeze(1), t.bool(), t.to(torch.uint8), t.to(torch.int32).unsqueeze(1), t.bool().unsqueeze(1)):
        assert torch.equal(crit(z, u), want)
    ti = t.clone()
    ti[0, 0] = -100
    assert torch.equal(crit(z, ti.to(torch.int32)), crit(z, ti))
    u8 = t.to(torch.uint8)
    u8[0, 0] = 255
    assert torch.equal(BinarySegLoss(ignore_index=255)(z, u8), BinarySegLoss()(z, ti))


@pytest.mark.parametrize("bad", [dict(bce=-1.0), dict(dice=-0.1), dict(focal_gamma=-1.0), dict(bce=float("inf")),
                                 dict(dice=float("nan")), dict(focal_gamma=float("inf")), dict(bce=0.0, dice=0.0),
                                 dict(pos_weight=0.0), dict(pos_weight=-1.0), dict(pos_weight=float("inf")),
                                 dict(dice_smooth=0.0), dict(dice_smooth=float("nan")), dict(threshold=0.0),
                                 dict(threshold=1.0), dict(threshold=-0.2), dict(threshold=float("nan"))])
def test_option_checks(bad):
    with pytest.raises(ValueError):
        BinarySegLoss(**bad)


def test_loss_options_binary_branch():
    dev = torch.device("cpu")
    opts = loss_options(None, 0.0, "mean", 1, dev, 0.6, 1.4, 1.5, 0.5, binary=True, pos_weight=2.5, threshold=0.3)
    assert opts[:3] == (None, 0.0, "mean")
    assert tuple(opts[3]) == (0.6, 1.4, 1.5, 0.5, 2.5, 0.3) and type(opts[3]).__name__ == "Binary"
    assert opts[3] != loss_options(None, 0.0, "mean", 1, dev, 0.6, 1.4, 1.5, 0.5, binary=True, pos_weight=2.0)[3]
    for kw in (dict(weight=torch.ones(1)), dict(label_smoothing=0.1), dict(reduction="sum"),
               dict(ohem_thresh=0.7, ohem_min_kept=16), dict(kd=1.0), dict(C=10), dict(C=2), dict(pos_weight=0.0),
               dict(threshold=1.0)):
        args = dict(weight=None, label_smoothing=0.0, reduction="mean", C=1, device=dev, binary=True)
        args.update(kw)
        with pytest.raises(ValueError):
            loss_options(**args)
    # the defaults are what they were: no Binary without binary=True
    assert loss_options(None, 0.0, "mean", 1, dev) == (None, 0.0, "mean", None)


def test_fused_loss_options():
    crit = BinarySegLoss(0.6, 1.4, 1.5, 2.5, ignore_index=255, dice_smooth=0.5, threshold=0.3)
    assert fused_loss_options(crit) == {"ignore_index": 255, "binary": True, "ce": 0.6, "dice": 1.4,
                                        "focal_gamma": 1.5, "dice_smooth": 0.5, "pos_weight": 2.5}

    class Mine(BinarySegLoss):
        def forward(self, logits, target):
            return super().forward(logits, target) * 2

    assert fused_loss_options(Mine()) is None
    assert fused_loss_options(nn.BCEWithLogitsLoss()) is None  # soft labels: the logits path


def test_saturated_logits():
    """|z| = 100 in fp32: everything finite.  1 - pt is exactly 0 only where exp(-|z|) underflows (|z| = 800 here, in
    fp32 and fp64 alike): there the focal factor, the term and its gradient are exactly 0, for gamma < 1 too."""
    t = torch.tensor([[[1, 0, 1, 0], [1, 0, 1, 0]]])
    for dtype in (torch.float32, torch.float64):
        z = torch.tensor([[[[100.0, -100.0, -100.0, 100.0], [800.0, -800.0, -800.0, 800.0]]]], dtype=dtype)
        for gamma in (0.0, 0.5, 2.0):
            zz = z.clone().requires_grad_(True)
            loss, focal, soft = binary_loss_terms(zz, t, 0.6, 1.4, gamma, 2.5, -100, 0.5)
            loss.backward()
            assert torch.isfinite(loss) and torch.isfinite(focal) and torch.isfinite(soft)
            assert torch.isfinite(zz.grad).all(), (dtype, gamma)
        # the pixels that are right beyond rounding: 1 - pt == 0
        sat, ts = z[:, :, 1:, :2].clone().requires_grad_(True), t[:, 1:, :2]
        assert torch.all(torch.sigmoid(-torch.where(ts == 1, sat[:, 0], -sat[:, 0])) == 0)
        for gamma in (0.5, 2.0):
            f = binary_loss_terms(sat, ts, 1.0, 0.0, gamma)[1]
            g, = torch.autograd.grad(f, sat)
            assert float(f) == 0.0 and torch.all(g == 0), (dtype, gamma)


def test_binary_summary():
    cm = torch.tensor([[50, 10], [5, 35]])
    s = binary_summary(cm)
    assert s["precision"] == 35 / 45 and s["recall"] == 35 / 40 and s["f1"] == 70 / 85
    s = binary_summary(torch.tensor([[7, 0], [0, 0]]))
    assert all(math.isnan(s[k]) for k in ("precision", "recall", "f1"))
    s = binary_summary(torch.tensor([[7, 0], [3, 0]]))
    assert math.isnan(s["precision"]) and s["recall"] == 0.0 and s["f1"] == 0.0
    with pytest.raises(ValueError):
        binary_summary(torch.zeros(3, 3, dtype=torch.int64))


def test_logit_threshold():
    assert logit_threshold(0.5) == 0.0
    z = logit_threshold(0.3)
    assert z == float(torch.tensor(math.log(0.3 / 0.7), dtype=torch.float64).float()) and z < 0 < logit_threshold(0.9)


@pytest.fixture(scope="module")
def val_case():
    """A LightUNet whose logits straddle both thresholds: the head's bias is set to the batch's median logit minus
    half the distance between zthr(0.3) and zthr(0.5), so some pixels lie between the two bounds."""
    model = deterministic_init(LightUNet(), seed=5).eval()
    g = torch.Generator().manual_seed(6)
    batches = [(torch.randn(2, 3, 32, 32, generator=g), torch.randint(0, 2, (2, 32, 32), generator=g))
               for _ in range(2)]
    batches[0][1][0, :3] = -100
    head = [m for m in model.modules() if isinstance(m, nn.Conv2d)][-1]
    with torch.no_grad():
        z = torch.cat([model(x)[:, 0].reshape(-1) for x, _ in batches])
        head.bias -= z.median() - 0.5 * logit_threshold(0.3)
        logits = [model(x) for x, _ in batches]
    return model, batches, logits


def bincount_matrix(logits, batches, zthr):
    cm = torch.zeros(2, 2, dtype=torch.int64)
    for z, (_, t) in zip(logits, batches):
        keep = t != -100
        cm += torch.bincount(t[keep] * 2 + (z[:, 0] > zthr)[keep].long(), minlength=4).reshape(2, 2)
    return cm


@pytest.mark.parametrize("fused", [True, False], ids=["forward_metrics", "criterion"])
def test_validate_on_a_one_logit_model(val_case, fused):
    model, batches, logits = val_case

    class Mine(BinarySegLoss):  # a forward of its own: validate() runs criterion(model(x), t)
        def forward(self, logits, target):
            return super().forward(logits, target)

    cls = BinarySegLoss if fused else Mine
    out = {}
    for thr in (0.5, 0.3):
        crit = cls(dice=0.5, pos_weight=2.0, threshold=thr)
        assert (fused_loss_options(crit) is not None) == fused
        res = validate(model, batches, crit, "cpu", progress=False)
        cm = res["confusion"]
        assert tuple(cm.shape) == (2, 2)
        assert torch.equal(cm, bincount_matrix(logits, batches, logit_threshold(thr)))
        assert int(cm.sum()) == sum(int((t != -100).sum()) for _, t in batches)
        want = binary_summary(cm)
        assert all(res[k] == want[k] for k in ("precision", "recall", "f1")) and not math.isnan(res["f1"])
        loss = sum(float(crit(z, t)) for z, (_, t) in zip(logits, batches)) / 2
        assert abs(res["loss"] - loss) < 1e-6 and len(res["iou"]) == 2
        out[thr] = cm
    # pixels with zthr(0.3) < z <= 0 exist by construction: the two thresholds cannot give the same matrix
    between = sum(int(((z[:, 0] > logit_threshold(0.3)) & (z[:, 0] <= 0) & (t != -100)).sum())
                  for z, (_, t) in zip(logits, batches))
    assert between > 0 and not torch.equal(out[0.5], out[0.3])
    assert int(out[0.3][:, 1].sum()) - int(out[0.5][:, 1].sum()) == between


def test_validate_rejects_tta_and_bad_labels(val_case):
    model, batches, _ = val_case
    with pytest.raises(ValueError):
        validate(model, batches, BinarySegLoss(), "cpu", progress=False, tta="hflip")
    x, t = batches[1]
    bad = t.clone()
    bad[0, 0, 0] = 2
    with pytest.raises(IndexError):
        validate(model, [(x, bad)], BinarySegLoss(), "cpu", progress=False)


def test_forward_loss_on_the_cpu(val_case):
    model, batches, logits = val_case
    x, t = batches[0]
    crit = BinarySegLoss(0.6, 1.4, 1.5, 2.5, dice_smooth=0.5)
    got = model.forward_loss(x, t, **fused_loss_options(crit))
    assert abs(float(got) - float(crit(logits[0], t))) < 1e-6
    x1, t1 = batches[1]  # nothing ignored: a bool [N, 1, H, W] mask is the same target
    assert torch.equal(model.forward_loss(x1, t1.bool().unsqueeze(1), binary=True, dice=0.5, pos_weight=2.0),
                       BinarySegLoss(dice=0.5, pos_weight=2.0)(logits[1], t1))
    assert abs(float(seg_amd.train.compute_loss(model, crit, x, t)) - float(got)) == 0.0
    with pytest.raises(ValueError):
        model.forward_loss(x, t, binary=True, label_smoothing=0.1)
    with pytest.raises(ValueError):
        model.forward_loss(x, t, binary=True, weight=torch.ones(1))


def test_exports():
    assert "BinarySegLoss" in seg_amd.__all__ and "binary_summary" in seg_amd.__all__


NEW_SYMBOLS = ["seg_bce_workspace_floats", "seg_bce_upsample_loss", "seg_bce_upsample_eval", "seg_bce_upsample_grad",
               "seg_bce_upsample_loss_bf16io", "seg_bce_upsample_eval_bf16io", "seg_bce_upsample_grad_bf16io",
               "seg_threshold_nearest"]


def test_new_symbols_are_declared_bound_and_exported():
    """tests/test_abi.py's rule, for the entry points this feature adds: declared in include/segamd.h, bound with the
    header's parameter types, exported by the built library, and invalid arguments rejected before any launch."""
    import ctypes
    from seg_amd import _lib
    from seg_amd.build import build, launchers
    decls = header_decls()
    taped = dict(launchers())
    for name in NEW_SYMBOLS:
        assert name in decls and name in _lib.PROTOTYPES, name
        ret, types = decls[name]
        res, args = _lib.PROTOTYPES[name]
        assert res == (ctypes.c_int if ret == "int" else ctypes.c_long) and [CTYPE[t] for t in types] == args, name
        assert name == "seg_bce_workspace_floats" or name in taped, name  # replayable from a launch tape
    # the gradient's one float per pixel in both maths: no row stride, a float* plane
    for name in ("seg_bce_upsample_grad", "seg_bce_upsample_grad_bf16io"):
        assert decls[name][1][-3:] == ["const float*", "float*", "hipStream_t"], decls[name]
    build()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.query("seg_bce_workspace_floats", 540800) == 6 * 2048
    assert _lib.query("seg_bce_workspace_floats", 100) == 6
    opts = (2.5, 1.0, 0.0, 0.0, 1.0)  # pos_weight, bce, dice, focal_gamma, dice_smooth
    loss = lambda ld, C, o: lib.seg_bce_upsample_loss(None, ld, 1, 4, 4, C, None, 8, 8, -100, *o, None, None, None)  # noqa: E731
    assert loss(4, 2, opts) == 1 and loss(4, 0, opts) == 1      # C must be 1
    assert loss(6, 1, opts) == 1                                 # ld & 3
    assert loss(4, 1, (0.0, 1.0, 0.0, 0.0, 1.0)) == 1            # pos_weight <= 0
    assert loss(4, 1, (-2.0, 1.0, 0.0, 0.0, 1.0)) == 1
    assert loss(4, 1, (1.0, 0.0, 0.0, 0.0, 1.0)) == 1            # bce and dice both 0
    assert loss(4, 1, (1.0, 1.0, 0.0, 0.0, 0.0)) == 1            # dice_smooth <= 0
    assert loss(4, 1, (1.0, 1.0, 0.0, float("nan"), 1.0)) == 1
    assert lib.seg_bce_upsample_eval(None, 4, 1, 4, 4, 1, None, 8, 8, -100, *opts, None, None, 0.0, None, None) == 1
    assert lib.seg_bce_upsample_grad(None, 4, 1, 4, 4, 2, None, 8, 8, -100, 2.5, 1.0, 0.0, 0.0, None, None, None,
                                     None) == 1
    assert lib.seg_bce_upsample_grad_bf16io(None, 6, 1, 4, 4, 1, None, 8, 8, -100, 2.5, 1.0, 0.0, 0.0, None, None,
                                            None, None) == 1
    assert lib.seg_threshold_nearest(None, 6, 1, 4, 4, 8, 8, 0.0, None, 16, 16, None) == 1
    assert lib.seg_threshold_nearest(None, 4, 1, 4, 4, 8, 8, float("nan"), None, 16, 16, None) == 1
