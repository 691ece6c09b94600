"""GPU: the weighted / smoothed fused loss kernels (csrc/loss.hip: seg_cew_upsample_loss / _grad /
_eval and their _bf16io twins) against F.cross_entropy in fp64 on the CPU over
F.interpolate(..., align_corners=True) of the same low-resolution logits, with the tolerances
tests/test_gpu_ops.py::test_ce_fused_upsample holds the plain kernels to; and bit for bit against
the plain kernels where the options say nothing (no weights or all ones, no smoothing, mean).
"""
import pytest
import torch
import torch.nn.functional as F

from seg_amd._lib import call, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
G = 0.7  # the upstream gradient

SHAPES = [(2, 10, 8, 16), (1, 4, 5, 7), (2, 1, 4, 4), (1, 21, 3, 5), (1, 32, 2, 3), (1, 10, 1, 1)]
WEIGHTS = ["none", "random", "zero_class"]
EPS = [0.0, 0.1, 1.0]
REDUCTIONS = ["mean", "sum"]


def S():
    return torch.cuda.current_stream().cuda_stream


def r4(c):
    return (c + 3) & ~3


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def nhwc(t, ld=None, dtype=torch.float32):
    """NCHW CPU tensor -> [N*H*W, ld] CUDA rows, the pad channels NaN (never read as data)."""
    N, C, H, W = t.shape
    ld = ld or r4(C)
    out = torch.full((N * H * W, ld), float("nan"), dtype=torch.float32)
    out[:, :C] = t.permute(0, 2, 3, 1).reshape(-1, C)
    return out.to(DEV, dtype)


def from_nhwc(rows, N, C, H, W):
    return rows[:, :C].float().reshape(N, H, W, C).permute(0, 3, 1, 2).cpu()


_CASES = {}


def case(N, C, H, W):
    """(low-resolution logits, labels with the first two rows of image 0 ignored): made once per shape."""
    key = (N, C, H, W)
    if key not in _CASES:
        low = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(1)) * 2
        y = torch.randint(0, C, (N, 2 * H, 2 * W), generator=torch.Generator().manual_seed(2))
        y[0, :2] = -100
        _CASES[key] = (low, y)
    return _CASES[key]


def weights(kind, C):
    if kind == "none":
        return None
    w = torch.rand(C, generator=torch.Generator().manual_seed(3)) * 3 + 0.05
    if kind == "zero_class":
        w[C // 2] = 0.0
    return w


_REFS = {}


def reference(shape, kind, eps, reduction):
    """fp64 CPU: (loss, gradient w.r.t. the low-resolution logits for upstream G, D, #valid)."""
    key = (shape, kind, eps, reduction)
    if key not in _REFS:
        N, C, H, W = shape
        low, y = case(*shape)
        w = weights(kind, C)
        lr = low.double().requires_grad_(True)
        z = F.interpolate(lr, size=(2 * H, 2 * W), mode="bilinear", align_corners=True)
        loss = F.cross_entropy(z, y, None if w is None else w.double(), reduction=reduction, label_smoothing=eps)
        loss.backward(torch.tensor(G, dtype=torch.float64))
        valid = y != -100
        wy = torch.ones(C, dtype=torch.float64) if w is None else w.double()
        D = float(wy[y[valid]].sum()) if reduction == "mean" else 1.0
        _REFS[key] = (loss.item(), lr.grad.clone(), D, int(valid.sum()))
    return _REFS[key]


def run_loss(lg, ld, N, H, W, C, yg, w=None, eps=0.0, reduction="mean", name="seg_cew_upsample_loss", conf=None):
    Ho, Wo = 2 * H, 2 * W
    out4 = torch.full((4,), -7.0, device=DEV)
    work = torch.empty(query("seg_cew_workspace_floats", N * Ho * Wo), device=DEV)
    args = [lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, w.data_ptr() if w is not None else None, eps,
            {"mean": 0, "sum": 1}[reduction], work.data_ptr(), out4.data_ptr()]
    if conf is not None:
        args.append(conf.data_ptr())
    call(name, *args, S())
    return out4


def run_grad(lg, ld, N, H, W, C, yg, stats, w=None, eps=0.0, name="seg_cew_upsample_grad", ldh=None, g=G,
             dtype=torch.float32):
    Ho, Wo = 2 * H, 2 * W
    ldh = ldh or r4(C)
    gout = torch.tensor([g], device=DEV)
    dhigh = torch.full((N * Ho * Wo, ldh), 5.0, device=DEV, dtype=dtype)
    call(name, lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, w.data_ptr() if w is not None else None,
         eps, gout.data_ptr(), stats.data_ptr(), dhigh.data_ptr(), ldh, S())
    return dhigh


def low_grad(dhigh, N, C, H, W, ldh=None):
    ldh = ldh or r4(C)
    if H == 1 and W == 1:  # every tap weight is 1 (seg_upsample_bwd's tap search divides by the zero scale)
        return dhigh[:, :r4(C)].float().reshape(N, -1, r4(C)).sum(1)
    dlow = torch.empty(N * H * W, r4(C), device=DEV)
    call("seg_upsample_bwd", dhigh.data_ptr(), ldh, 0, N, 2 * H, 2 * W, C, dlow.data_ptr(), r4(C), H, W, 1, 0, S())
    return dlow


def check_against_reference(shape, kind, eps, reduction, out4, dlow):
    N, C, H, W = shape
    loss, grad, D, nvalid = reference(shape, kind, eps, reduction)
    o = out4.cpu().double().tolist()
    tag = (shape, kind, eps, reduction, o, loss)
    assert o[3] == nvalid and o[2] == 0, tag
    if reduction == "sum":
        assert o[1] == 1.0, tag
    else:
        assert abs(o[1] - D) <= 1e-5 * abs(D) + 1e-7, tag
    if loss != loss:  # D == 0 under mean reduction: 0/0, as aten
        assert o[0] != o[0], tag
    else:
        assert abs(o[0] - loss) <= 1e-5 * abs(loss) + 1e-7, tag
    got = from_nhwc(dlow, N, C, H, W)
    if not torch.isfinite(grad).all():
        assert not torch.isfinite(got).all(), tag
    elif float(grad.abs().max()) == 0.0:
        assert float(got.abs().max()) <= 1e-7, tag
    else:
        assert rel(got, grad) < 1e-5, (tag, rel(got, grad))


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradient_against_fp64(shape, kind):
    N, C, H, W = shape
    low, y = case(*shape)
    lg, yg = nhwc(low), y.to(DEV)
    w = weights(kind, C)
    wg = None if w is None else w.to(DEV)
    for eps in EPS:
        for reduction in REDUCTIONS:
            out4 = run_loss(lg, r4(C), N, H, W, C, yg, wg, eps, reduction)
            dhigh = run_grad(lg, r4(C), N, H, W, C, yg, out4, wg, eps)
            assert torch.all(dhigh[:, C:] == 0)
            check_against_reference(shape, kind, eps, reduction, out4, low_grad(dhigh, N, C, H, W))


def test_zero_weight_on_the_only_class_is_nan_like_aten():
    shape = (2, 1, 4, 4)
    loss, _, D, _ = reference(shape, "zero_class", 0.1, "mean")
    assert loss != loss and D == 0.0
    low, y = case(*shape)
    out4 = run_loss(nhwc(low), 4, 2, 4, 4, 1, y.to(DEV), weights("zero_class", 1).to(DEV), 0.1, "mean")
    assert torch.isnan(out4[0]) and out4[1].item() == 0 and out4[2].item() == 0
    out4 = run_loss(nhwc(low), 4, 2, 4, 4, 1, y.to(DEV), weights("zero_class", 1).to(DEV), 0.1, "sum")
    assert out4[0].item() == 0.0 and out4[1].item() == 1.0


@pytest.mark.parametrize("io", ["f32", "bf16io"])
@pytest.mark.parametrize("shape", SHAPES)
def test_no_options_is_the_plain_kernel_bit_for_bit(shape, io):
    N, C, H, W = shape
    Ho, Wo = 2 * H, 2 * W
    low, y = case(*shape)
    dtype, sfx = (torch.float32, "") if io == "f32" else (BF, "_bf16io")
    lg, yg = nhwc(low.to(BF).float(), dtype=dtype), y.to(DEV)
    ld = r4(C)
    out3 = torch.empty(3, device=DEV)
    work = torch.empty(query("seg_ce_workspace_floats", N * Ho * Wo), device=DEV)
    call("seg_ce_upsample_loss" + sfx, lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, work.data_ptr(),
         out3.data_ptr(), S())
    gout = torch.tensor([G], device=DEV)
    plain = torch.full((N * Ho * Wo, ld), 5.0, device=DEV, dtype=dtype)
    call("seg_ce_upsample_grad" + sfx, lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, gout.data_ptr(),
         out3.data_ptr(), plain.data_ptr(), ld, S())
    for w in (None, torch.ones(C, device=DEV)):
        out4 = run_loss(lg, ld, N, H, W, C, yg, w, 0.0, "mean", "seg_cew_upsample_loss" + sfx)
        assert torch.equal(out4[:3], out3) or (torch.isnan(out3[0]) and torch.isnan(out4[0])
                                               and torch.equal(out4[1:3], out3[1:])), (out4, out3)
        dhigh = run_grad(lg, ld, N, H, W, C, yg, out4, w, 0.0, "seg_cew_upsample_grad" + sfx, dtype=dtype)
        assert torch.equal(dhigh, plain)


@pytest.mark.parametrize("shape", [(2, 10, 8, 16), (1, 21, 3, 5), (1, 32, 2, 3)])
def test_eval_is_the_loss_plus_the_plain_confusion_matrix(shape):
    N, C, H, W = shape
    Ho, Wo = 2 * H, 2 * W
    low, y = case(*shape)
    lg, yg = nhwc(low), y.to(DEV)
    ld = r4(C)
    ref = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    out3 = torch.empty(3, device=DEV)
    work = torch.empty(query("seg_ce_workspace_floats", N * Ho * Wo), device=DEV)
    call("seg_ce_upsample_eval", lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, work.data_ptr(),
         out3.data_ptr(), ref.data_ptr(), S())
    assert int(ref.sum()) == int((y != -100).sum())
    for kind in WEIGHTS:
        w = weights(kind, C)
        wg = None if w is None else w.to(DEV)
        for eps, reduction in ((0.0, "mean"), (0.1, "mean"), (1.0, "sum")):
            conf = torch.zeros(C * C + 8, dtype=torch.int64, device=DEV)
            o_eval = run_loss(lg, ld, N, H, W, C, yg, wg, eps, reduction, "seg_cew_upsample_eval", conf)
            o_loss = run_loss(lg, ld, N, H, W, C, yg, wg, eps, reduction)
            assert torch.equal(o_eval.view(torch.int32), o_loss.view(torch.int32))
            assert torch.equal(conf[:C * C].reshape(C, C), ref) and torch.all(conf[C * C:] == 0)
            run_loss(lg, ld, N, H, W, C, yg, wg, eps, reduction, "seg_cew_upsample_eval", conf)  # accumulates
            assert torch.equal(conf[:C * C].reshape(C, C), 2 * ref) and torch.all(conf[C * C:] == 0)


def test_bf16io_twins():
    """As test_gpu_bf16io.py::test_cross_entropy: the twins on bf16 logits, the fp32 entries on the same values
    widened -- identical stats, and the gradient is the fp32 gradient rounded once to bf16."""
    N, C, H, W = 2, 10, 16, 32
    Ho, Wo = 2 * H, 2 * W
    x = (torch.randn(N * H * W, 12, generator=torch.Generator().manual_seed(12)) * 2).to(BF)
    lo32, lo16 = x.float().to(DEV), x.to(DEV)
    t = torch.randint(0, C, (N, Ho, Wo), generator=torch.Generator().manual_seed(13)).to(DEV)
    t[0, :3] = -100
    w = weights("zero_class", C).to(DEV)
    for eps, reduction in ((0.1, "mean"), (0.0, "sum")):
        st32 = run_loss(lo32, 12, N, H, W, C, t, w, eps, reduction)
        st16 = run_loss(lo16, 12, N, H, W, C, t, w, eps, reduction, "seg_cew_upsample_loss_bf16io")
        assert torch.equal(st32, st16) and torch.isfinite(st32).all()
        conf32 = torch.zeros(C * C, dtype=torch.int64, device=DEV)
        conf16 = torch.zeros(C * C, dtype=torch.int64, device=DEV)
        e32 = run_loss(lo32, 12, N, H, W, C, t, w, eps, reduction, "seg_cew_upsample_eval", conf32)
        e16 = run_loss(lo16, 12, N, H, W, C, t, w, eps, reduction, "seg_cew_upsample_eval_bf16io", conf16)
        assert torch.equal(e32, st32) and torch.equal(e16, st32) and torch.equal(conf32, conf16)
        d32 = run_grad(lo32, 12, N, H, W, C, t, st32, w, eps, g=1.0)
        d16 = run_grad(lo16, 12, N, H, W, C, t, st16, w, eps, "seg_cew_upsample_grad_bf16io", g=1.0, dtype=BF)
        assert torch.equal(d16.view(torch.int16), d32.to(BF).view(torch.int16))


@pytest.mark.parametrize("bad", [10, 255, -1])
def test_out_of_range_label(bad):
    N, C, H, W = 1, 10, 4, 6
    low = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(1))
    y = torch.randint(0, C, (N, 2 * H, 2 * W), generator=torch.Generator().manual_seed(3))
    y[0, 1, 2] = bad
    lg, yg = nhwc(low), y.to(DEV)
    w = weights("random", C).to(DEV)
    for reduction in REDUCTIONS:
        out4 = run_loss(lg, 12, N, H, W, C, yg, w, 0.1, reduction)
        assert out4[2].item() == 1 and torch.isnan(out4[0]) and out4[3].item() == y.numel() - 1
        dhigh = run_grad(lg, 12, N, H, W, C, yg, out4, w, 0.1, g=1.0)
        assert torch.isnan(dhigh[:, :C]).any() and torch.all(dhigh[:, C:] == 0)


def test_row_strides():
    """ld = 16 for C = 10 (a channel slice of a wider buffer), and a dhigh row stride other than the logits'."""
    shape = (2, 10, 8, 16)
    N, C, H, W = shape
    low, y = case(*shape)
    yg = y.to(DEV)
    w = weights("random", C).to(DEV)
    lg16, lg12 = nhwc(low, 16), nhwc(low, 12)
    o16 = run_loss(lg16, 16, N, H, W, C, yg, w, 0.1, "mean")
    o12 = run_loss(lg12, 12, N, H, W, C, yg, w, 0.1, "mean")
    assert torch.equal(o16, o12)
    d12 = run_grad(lg12, 12, N, H, W, C, yg, o12, w, 0.1)
    check_against_reference(shape, "random", 0.1, "mean", o12, low_grad(d12, N, C, H, W))
    d16 = run_grad(lg16, 16, N, H, W, C, yg, o16, w, 0.1, ldh=16)        # ld = ldh = 16
    dmix = run_grad(lg12, 12, N, H, W, C, yg, o12, w, 0.1, ldh=16)       # ld = 12, ldh = 16
    for d in (d16, dmix):
        assert torch.equal(d[:, :12], d12)
        assert torch.all(d[:, 12:] == 5.0)  # behind round4(C): not this kernel's to write
    check_against_reference(shape, "random", 0.1, "mean", o12, low_grad(dmix, N, C, H, W, ldh=16))
