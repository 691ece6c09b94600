"""GPU: the fused validation kernel (seg_ce_upsample_eval: loss + argmax + confusion matrix from
the low-resolution logits, csrc/loss.hip), the engine's "metrics" mode behind
`model.forward_metrics`, and `seg_amd.validate` on the device.

The reference of every kernel case is torch on the CPU in fp64 from the same low-resolution
logits: F.interpolate(align_corners=True), argmax(1), bincount, F.cross_entropy.

Where logits are generic floats, a pixel whose two best fp64 logits lie closer than MARGIN may
legitimately flip in fp32 (the recomputed logits carry ~1e-6 of rounding at |z| <= 5, two
orders below MARGIN): such pixels are left out of the comparison by giving them the ignore
label, and their share is bounded by MAX_LEFT_OUT (the fp64 reference alone leaves out 0 of 480 and
5 of 16384 pixels of the two generic cases).  The exact
case needs no margin: every interpolated value is exact in fp32, ties included.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from seg_amd._lib import call, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
MARGIN = 1e-4
MAX_LEFT_OUT = 0.005
GUARD = 64  # int64 words behind the C*C matrix that must stay untouched


def r4(c):
    return (c + 3) & ~3


def S():
    return torch.cuda.current_stream().cuda_stream


def rows(low, ld=None, fill=float("nan")):
    """NCHW CPU logits -> [N*H*W, ld] CUDA rows; the lanes C..ld-1 hold `fill`."""
    N, C, H, W = low.shape
    ld = ld or r4(C)
    out = torch.full((N * H * W, ld), fill, dtype=torch.float32)
    out[:, :C] = low.permute(0, 2, 3, 1).reshape(-1, C)
    return out.to(DEV)


def reference(low, y, Ho, Wo, ignore_index=-100):
    """fp64 CPU: (confusion [C, C], loss or None when a label is out of range, #valid, #bad, top-2 margin)."""
    C = low.shape[1]
    z = F.interpolate(low.double(), size=(Ho, Wo), mode="bilinear", align_corners=True)
    pred = z.argmax(1)
    bad = (y != ignore_index) & ((y < 0) | (y >= C))
    keep = (y != ignore_index) & ~bad
    cm = torch.bincount(y[keep] * C + pred[keep], minlength=C * C).reshape(C, C)
    loss = None
    if not bad.any():
        loss = F.cross_entropy(z, y, ignore_index=ignore_index).item()
    if C > 1:
        top = z.topk(2, dim=1).values
        margin = top[:, 0] - top[:, 1]
    else:
        margin = torch.full(y.shape, float("inf"), dtype=torch.float64)
    return cm, loss, int(keep.sum()), int(bad.sum()), margin


def run_eval(lg, ld, N, H, W, C, y, Ho, Wo, ignore_index=-100, confusion=None, name="seg_ce_upsample_eval"):
    """One call of the eval entry point: (confusion [C, C] on the CPU, out3 on the device).  The
    matrix buffer carries GUARD extra words, checked to be untouched."""
    yg = y.to(DEV)
    out3 = torch.empty(3, device=DEV)
    work = torch.empty(query("seg_ce_workspace_floats", N * Ho * Wo), device=DEV)
    buf = torch.zeros(C * C + GUARD, dtype=torch.int64, device=DEV) if confusion is None else confusion
    call(name, lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, ignore_index, work.data_ptr(),
         out3.data_ptr(), buf.data_ptr(), S())
    torch.cuda.synchronize()
    assert torch.all(buf[C * C:] == 0), "counts landed behind the C*C matrix"
    return buf[:C * C].reshape(C, C).cpu(), out3


def run_loss(lg, ld, N, H, W, C, y, Ho, Wo, ignore_index=-100, name="seg_ce_upsample_loss"):
    yg = y.to(DEV)
    out3 = torch.empty(3, device=DEV)
    work = torch.empty(query("seg_ce_workspace_floats", N * Ho * Wo), device=DEV)
    call(name, lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, ignore_index, work.data_ptr(),
         out3.data_ptr(), S())
    torch.cuda.synchronize()
    return out3


def bitwise(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def int_logits(N, C, H, W, seed):
    return torch.randint(-3, 4, (N, C, H, W), generator=torch.Generator().manual_seed(seed)).float()


def labels(N, C, Ho, Wo, seed):
    return torch.randint(0, C, (N, Ho, Wo), generator=torch.Generator().manual_seed(seed))


def test_exact_case_with_ties():
    """Scale (H-1)/(Ho-1) = 1/2 and integer logits: every interpolated logit is a multiple of 1/4,
    exact in fp32, so the matrix must EQUAL the fp64 reference's -- including the many pixels whose
    best logit is shared by several classes, which pins the lowest-index tie rule."""
    N, C, H, W, Ho, Wo = 2, 10, 5, 9, 9, 17
    low, y = int_logits(N, C, H, W, 1), labels(N, C, Ho, Wo, 2)
    cm, loss, valid, _, margin = reference(low, y, Ho, Wo)
    ties = int((margin == 0).sum())
    print(f"exact ties: {ties} of {N * Ho * Wo} pixels")
    assert ties >= N * Ho * Wo // 10, "the case must contain ties to pin the rule"
    got, out3 = run_eval(rows(low), r4(C), N, H, W, C, y, Ho, Wo)
    assert torch.equal(got, cm)
    assert out3[1].item() == valid == int(got.sum()) and out3[2].item() == 0
    assert abs(out3[0].item() - loss) <= 1e-5 * abs(loss) + 1e-7


@pytest.mark.parametrize("C,ld", [(10, 16), (1, 4), (32, 36)])
def test_padding_lanes_never_win(C, ld):
    """The lanes C..ld-1 hold +100 (above every real logit): a prediction must still be a real class."""
    N, H, W, Ho, Wo = 2, 5, 9, 9, 17
    low, y = int_logits(N, C, H, W, 3), labels(N, C, Ho, Wo, 4)
    cm, loss, valid, _, _ = reference(low, y, Ho, Wo)
    got, out3 = run_eval(rows(low, ld, 100.0), ld, N, H, W, C, y, Ho, Wo)
    assert torch.equal(got, cm)
    assert int(got.sum()) == valid == N * Ho * Wo
    assert abs(out3[0].item() - loss) <= 1e-5 * abs(loss) + 1e-7


@pytest.mark.parametrize("H,W", [(6, 10), (32, 64)])
def test_generic_x2(H, W):
    N, C, Ho, Wo = 2, 10, 2 * H, 2 * W
    low = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(5))
    y = labels(N, C, Ho, Wo, 6)
    _, loss, _, _, margin = reference(low, y, Ho, Wo)
    close = margin < MARGIN
    share = close.float().mean().item()
    print(f"left out (fp64 top-2 margin < {MARGIN}): {int(close.sum())} of {close.numel()}")
    assert share <= MAX_LEFT_OUT
    yk = torch.where(close, torch.full_like(y, -100), y)
    cm, _, valid, _, _ = reference(low, yk, Ho, Wo)
    lg = rows(low)
    got, _ = run_eval(lg, r4(C), N, H, W, C, yk, Ho, Wo)
    assert torch.equal(got, cm) and int(got.sum()) == valid
    # the loss, on the full label map: test_gpu_ops.py's tolerance for seg_ce_upsample_loss, and the same bits
    _, out3 = run_eval(lg, r4(C), N, H, W, C, y, Ho, Wo)
    assert abs(out3[0].item() - loss) <= 1e-5 * abs(loss) + 1e-7
    assert bitwise(out3, run_loss(lg, r4(C), N, H, W, C, y, Ho, Wo))


@pytest.mark.parametrize("ignore_index", [-100, 255])
def test_ignored_and_out_of_range_labels(ignore_index):
    N, C, H, W, Ho, Wo = 2, 10, 5, 9, 9, 17
    low, y = int_logits(N, C, H, W, 7), labels(N, C, Ho, Wo, 8)
    y[0, :2] = ignore_index
    y[1, 3, 4:9] = ignore_index
    lg = rows(low)
    cm, loss, valid, _, _ = reference(low, y, Ho, Wo, ignore_index)
    got, out3 = run_eval(lg, r4(C), N, H, W, C, y, Ho, Wo, ignore_index)
    assert torch.equal(got, cm) and int(got.sum()) == valid == out3[1].item()
    assert out3[2].item() == 0 and abs(out3[0].item() - loss) <= 1e-5 * abs(loss) + 1e-7
    y[1, 5, 5] = C  # aten raises "Target out of bounds": counted, in no bin, NaN loss
    cm, _, valid, bad, _ = reference(low, y, Ho, Wo, ignore_index)
    got, out3 = run_eval(lg, r4(C), N, H, W, C, y, Ho, Wo, ignore_index)
    assert bad == 1 and out3[2].item() == 1 and torch.isnan(out3[0])
    assert torch.equal(got, cm) and int(got.sum()) == valid == out3[1].item()
    loss3 = run_loss(lg, r4(C), N, H, W, C, y, Ho, Wo, ignore_index)
    assert bitwise(out3, loss3)
    # everything ignored: 0/0, as aten
    got, out3 = run_eval(lg, r4(C), N, H, W, C, torch.full_like(y, ignore_index), Ho, Wo, ignore_index)
    assert int(got.sum()) == 0 and torch.isnan(out3[0]) and out3[1].item() == 0


def test_accumulates_into_the_buffer():
    N, C, H, W, Ho, Wo = 2, 10, 5, 9, 9, 17
    la, ya = int_logits(N, C, H, W, 9), labels(N, C, Ho, Wo, 10)
    lb, yb = int_logits(N, C, H, W, 11), labels(N, C, Ho, Wo, 12)
    a, _ = run_eval(rows(la), r4(C), N, H, W, C, ya, Ho, Wo)
    b, _ = run_eval(rows(lb), r4(C), N, H, W, C, yb, Ho, Wo)
    buf = torch.zeros(C * C + GUARD, dtype=torch.int64, device=DEV)
    run_eval(rows(la), r4(C), N, H, W, C, ya, Ho, Wo, confusion=buf)
    both, _ = run_eval(rows(lb), r4(C), N, H, W, C, yb, Ho, Wo, confusion=buf)
    assert torch.equal(both, a + b)


def test_capped_grid_loops():
    """N*Ho*Wo = 525825 > 2048 blocks * 256 threads: the grid-stride loop takes a second trip."""
    N, C, H, W, Ho, Wo = 1, 10, 257, 513, 513, 1025
    assert 2048 * 256 < N * Ho * Wo < 2 * 2048 * 256
    low = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(13))
    y = labels(N, C, Ho, Wo, 14)
    y[0, -1, -7:] = -100
    _, loss, _, _, margin = reference(low, y, Ho, Wo)
    close = margin < MARGIN
    assert close.float().mean().item() <= MAX_LEFT_OUT
    yk = torch.where(close, torch.full_like(y, -100), y)
    cm, _, valid, _, _ = reference(low, yk, Ho, Wo)
    lg = rows(low)
    got, out3 = run_eval(lg, r4(C), N, H, W, C, yk, Ho, Wo)
    assert int(got.sum()) == valid == out3[1].item()
    assert torch.equal(got, cm)
    _, out3 = run_eval(lg, r4(C), N, H, W, C, y, Ho, Wo)
    assert abs(out3[0].item() - loss) <= 1e-5 * abs(loss) + 1e-7
    assert bitwise(out3, run_loss(lg, r4(C), N, H, W, C, y, Ho, Wo))


def test_bf16io_entry_point():
    N, C, H, W, Ho, Wo = 2, 10, 6, 10, 12, 20
    low = (torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(15)) * 2).to(BF).float()
    y = labels(N, C, Ho, Wo, 16)
    y[0, :2] = -100
    lg32 = rows(low, 12, 100.0)
    lg16 = lg32.to(BF)
    assert torch.equal(lg16.float(), lg32)
    c32, o32 = run_eval(lg32, 12, N, H, W, C, y, Ho, Wo)
    c16, o16 = run_eval(lg16, 12, N, H, W, C, y, Ho, Wo, name="seg_ce_upsample_eval_bf16io")
    assert torch.equal(c16, c32) and bitwise(o16, o32)
    assert bitwise(o16, run_loss(lg16, 12, N, H, W, C, y, Ho, Wo, name="seg_ce_upsample_loss_bf16io"))


def test_null_confusion_is_rejected_before_any_launch():
    import ctypes
    from seg_amd import _lib
    rc = _lib.lib().seg_ce_upsample_eval(None, 12, 1, 4, 4, 10, None, 8, 8, -100, None, None, None, None)
    assert rc == 1
    rc = _lib.lib().seg_ce_upsample_eval(None, 10, 1, 4, 4, 10, None, 8, 8, -100, None, None, ctypes.c_void_p(8), None)
    assert rc == 1  # ld not a multiple of 4


# ---------------------------------------------------------------------------- model level
def _models():
    from seg_amd import MobileNetV2UNet, UNet
    return {"mnv2": (lambda: MobileNetV2UNet(10), 10, (2, 3, 64, 128)),
            "unet": (lambda: UNet(4, 64), 4, (2, 3, 32, 64))}


@pytest.mark.parametrize("arch", ["mnv2", "unet"])
def test_forward_metrics_matches_the_logits_path(arch):
    from seg_amd import deterministic_init
    ctor, C, shape = _models()[arch]
    model = deterministic_init(ctor(), seed=3).to(DEV).eval()
    N, _, H, W = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(17)).to(DEV)
    y = labels(N, C, H, W, 18)
    y[0, :3] = -100
    with torch.no_grad():
        logits = model(x)
    top = logits.topk(2, dim=1).values
    close = ((top[:, 0] - top[:, 1]) < MARGIN).cpu()
    share = close.float().mean().item()
    print(f"{arch}: left out (fp32 top-2 margin < {MARGIN}): {int(close.sum())} of {close.numel()}")
    assert share <= MAX_LEFT_OUT
    yk = torch.where(close, torch.full_like(y, -100), y).to(DEV)
    keep = yk != -100
    want = torch.bincount(yk[keep] * C + logits.argmax(1)[keep], minlength=C * C).reshape(C, C)
    conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    loss = model.forward_metrics(x, yk, conf)
    assert not loss.requires_grad
    assert torch.equal(conf, want)
    ref = F.cross_entropy(logits, yk).item()
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref) + 1e-7
    # the second call replays the recorded tape and accumulates
    loss2 = model.forward_metrics(x, yk, conf)
    assert torch.equal(conf, 2 * want) and loss2.item() == loss.item()
    assert not model.training  # the mode is the caller's
    # the fused training loss of the same eval-mode model is the same number (same kernel order)
    with torch.no_grad():
        assert model.forward_loss(x, yk).item() == loss.item()


def test_forward_metrics_reports_bad_labels():
    from seg_amd import MobileNetV2UNet, deterministic_init
    from seg_amd.engine import check_targets
    model = deterministic_init(MobileNetV2UNet(10), seed=3).to(DEV).eval()
    x = torch.randn(2, 3, 64, 128, generator=torch.Generator().manual_seed(19)).to(DEV)
    y = labels(2, 10, 64, 128, 20).to(DEV)
    y[1, 7, 7] = 10
    conf = torch.zeros(10, 10, dtype=torch.int64, device=DEV)
    loss = model.forward_metrics(x, y, conf)
    assert torch.isnan(loss) and int(conf.sum()) == y.numel() - 1
    with pytest.raises(IndexError, match="Target out of bounds"):
        check_targets(model)
    with pytest.raises(ValueError):
        model.forward_metrics(x, y, torch.zeros(10, 10, dtype=torch.int32, device=DEV))


def test_validate_on_the_gpu():
    from seg_amd import MobileNetV2UNet, deterministic_init, summarize, validate
    model = deterministic_init(MobileNetV2UNet(10), seed=3).to(DEV).train()
    loader = []
    for k in range(3):
        x = torch.randn(2, 3, 64, 128, generator=torch.Generator().manual_seed(30 + k))
        y = labels(2, 10, 64, 128, 40 + k)
        y[0, k] = -100
        loader.append((x, y))
    crit = nn.CrossEntropyLoss()
    out = validate(model, loader, crit, DEV, progress=False)
    assert model.training  # restored
    model.eval()
    total = torch.zeros(10, 10, dtype=torch.int64, device=DEV)
    losses = []
    for x, y in loader:
        losses.append(model.forward_metrics(x.to(DEV), y.to(DEV), total).item())
    want = summarize(total)
    assert torch.equal(out["confusion"], want["confusion"])
    assert out["miou"] == want["miou"] and out["pixel_acc"] == want["pixel_acc"]
    assert torch.equal(out["iou"].isnan(), want["iou"].isnan())
    assert torch.equal(out["iou"].nan_to_num(-1), want["iou"].nan_to_num(-1))
    assert out["loss"] == sum(losses) / 3
    # an unfusable criterion takes the device fallback: same matrix away from argmax near-ties, same loss
    fb = validate(model, loader, nn.CrossEntropyLoss(label_smoothing=0.0, weight=torch.ones(10, device=DEV)), DEV,
                  progress=False)
    assert abs(fb["loss"] - out["loss"]) <= 1e-5 * abs(out["loss"])
    differ = int((fb["confusion"] - out["confusion"]).abs().sum()) // 2
    assert differ <= MAX_LEFT_OUT * int(out["confusion"].sum())
    # a bad label raises at the end of the pass
    loader[1][1][1, 9, 9] = 10
    with pytest.raises(IndexError, match="Target out of bounds"):
        validate(model, loader, crit, DEV, progress=False)
