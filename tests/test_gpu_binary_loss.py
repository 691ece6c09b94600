"""GPU: the one-logit fused loss kernels (csrc/loss.hip: seg_bce_upsample_loss / _eval / _grad and their _bf16io
twins) and seg_threshold_nearest (csrc/infer.hip) against seg_amd.losses.binary_loss_terms in fp64 on the CPU over
F.interpolate(..., align_corners=True) of the same low-resolution logits, upstream gradient 0.7.

Tolerance: the one tests/test_gpu_loss_options.py and tests/test_gpu_seg_loss.py hold the other families to -- 1e-5
relative (+1e-7) on loss, F and Dice, 1e-5 relative norm on the low-resolution gradient (after seg_upsample_bwd with
nchw_grad = 1, ac = 2).  Where a case misses that, its bound is 4x the error of the same torch composition run in fp32
on the CPU against fp64; every such case is written through the `record` fixture.

Confusion matrix: pixels whose fp64 logit lies within MARGIN of the threshold's logit get the ignore label (their
share is bounded by MAX_LEFT_OUT); the matrix must then equal the fp64 one exactly.  The tie case has no margin: its
logits are exact in fp32.

Measured on an MI355X (profiles/binary_parity.jsonl): the five small shapes are inside the 1e-5 target in every
option set, row stride and math (loss, F, Dice within 1.7e-7, gradient within 1.5e-7; logits x 30: 8.3e-8 and 1.1e-6).
On (1, 1, 260, 520) -> (520, 1040) the loss terms are within 1.7e-6 and the gradient at 8.3e-6 .. 9.6e-6 for four of
the five option sets, inside the target; the one fallback is gamma = 0.5 there (ld 4, ld 8 and bf16io alike), whose
gradient is at 1.029e-5 against a fallback bound of 6.96e-5 (4x the CPU's fp32 composition, 1.74e-5).  The same
gradient plane behind seg_upsample_bwd(ac = 1) instead of ac = 2 is at 1.34e-5 for the "all" set (ac = 2: 8.25e-6).
The confusion matrix leaves out 0 pixels on the small shapes and 29 / 30 / 8 of 540 800 on the big one (thresholds
0.5 / 0.3 / 0.9) and then equals the fp64 one exactly; seg_threshold_nearest leaves out at most 1 model pixel.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cvresize
from seg_amd._lib import call, lib, query
from seg_amd.losses import binary_loss_terms, logit_threshold

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
G = 0.7  # the upstream gradient
TOL = 1e-5
MARGIN = 1e-4
MAX_LEFT_OUT = 0.005
GUARD = 16
SENTINEL = -7.0

BIG = ((1, 1, 260, 520), (520, 1040))  # 540 800 output pixels > 2048 x 256: the grid-stride loop, all 2048 partials
SMALL = [((2, 1, 4, 4), (8, 8)), ((1, 1, 5, 7), (10, 14)), ((1, 1, 3, 5), (6, 10)),
         ((1, 1, 1, 1), (2, 2)),     # one source pixel, scale 0, and every pixel ignored
         ((1, 1, 5, 9), (9, 17))]    # not x2
SHAPES = SMALL + [BIG]
IDS = lambda s: "x".join(map(str, s[0])) + "to" + "x".join(map(str, s[1]))  # noqa: E731
CASES = {"bce": dict(bce=1.0, dice=0.0, focal_gamma=0.0, pos_weight=2.5, dice_smooth=1.0),
         "gamma0.5": dict(bce=1.0, dice=0.0, focal_gamma=0.5, pos_weight=1.0, dice_smooth=1.0),
         "gamma2": dict(bce=1.0, dice=0.0, focal_gamma=2.0, pos_weight=1.0, dice_smooth=1.0),
         "dice": dict(bce=0.0, dice=1.0, focal_gamma=0.0, pos_weight=1.0, dice_smooth=1.0),
         "all": dict(bce=0.6, dice=1.4, focal_gamma=1.5, pos_weight=2.5, dice_smooth=0.5)}
THRESHOLDS = [0.5, 0.3, 0.9]


def S():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def rows(low, ld=4, dtype=torch.float32):
    """[N, 1, H, W] CPU logits -> [N*H*W, ld] CUDA rows (a channel-slice view for ld = 8), the pad lanes NaN."""
    out = torch.full((low.numel(), ld), float("nan"), dtype=torch.float32)
    out[:, 0] = low.reshape(-1)
    return out.to(DEV, dtype)


_CASES = {}


def case(shape, out_hw, scale=1.0):
    """(low-resolution logits randn(seed 1) * 2, labels randint(0, 2, seed 2) with the first two rows of image 0
    ignored): made once per shape."""
    key = (shape, out_hw, scale)
    if key not in _CASES:
        N = shape[0]
        low = torch.randn(*shape, generator=torch.Generator().manual_seed(1)) * 2 * scale
        y = torch.randint(0, 2, (N, *out_hw), generator=torch.Generator().manual_seed(2))
        y[0, :2] = -100
        _CASES[key] = (low, y)
    return _CASES[key]


def upsample64(low, out_hw):
    return F.interpolate(low.double(), size=out_hw, mode="bilinear", align_corners=True)


def composition(low, y, opts, dtype):
    """binary_loss_terms over the interpolated logits in `dtype` on the CPU: loss, F, Dice, low-res gradient."""
    lr = low.detach().to(dtype).clone().requires_grad_(True)
    z = F.interpolate(lr, size=tuple(y.shape[1:]), mode="bilinear", align_corners=True)
    loss, focal, dice = binary_loss_terms(z, y, **opts)
    loss.backward(torch.tensor(G, dtype=dtype))
    f = lambda t: None if t is None else float(t.detach())  # noqa: E731
    return f(loss), f(focal), f(dice), lr.grad.double()


_REFS = {}


def reference(low, y, name, key):
    """fp64 CPU: dict(loss, F, Dice, grad, nvalid, a, b).  Made once per case and shared."""
    key = (key, name)
    if key not in _REFS:
        opts = CASES[name]
        loss, focal, dice, grad = composition(low, y, opts, torch.float64)
        valid = y != -100
        with torch.no_grad():
            s = torch.sigmoid(upsample64(low, tuple(y.shape[1:]))[:, 0])
            Ssum, I, T = float(s[valid].sum()), float(s[valid & (y == 1)].sum()), float((valid & (y == 1)).sum())
        U = Ssum + T + opts["dice_smooth"]
        _REFS[key] = dict(loss=loss, F=focal, Dice=dice, grad=grad, nvalid=int(valid.sum()), a=2.0 / U,
                          b=(2.0 * I + opts["dice_smooth"]) / (U * U), low=low, y=y, opts=opts)
    return _REFS[key]


def fp32_bounds(ref):
    """4x the error of the same composition in fp32 on the CPU against fp64: (loss bound, gradient bound)."""
    if "bounds" not in ref:
        loss, _, _, grad = composition(ref["low"], ref["y"], ref["opts"], torch.float32)
        e_loss = abs(loss - ref["loss"]) / max(abs(ref["loss"]), 1e-30) if ref["loss"] == ref["loss"] else 0.0
        e_grad = rel(grad, ref["grad"]) if torch.isfinite(ref["grad"]).all() else 0.0
        ref["bounds"] = (4 * e_loss, 4 * e_grad)
    return ref["bounds"]


def guarded(n, dtype=torch.float32, fill=SENTINEL):
    """n words to write and GUARD words behind them that must stay as they are."""
    return torch.full((n + GUARD,), fill, device=DEV, dtype=dtype)


def guard_ok(buf, n, fill=SENTINEL):
    return bool(torch.all(buf[n:] == fill))


def run_loss(lg, ld, shape, yg, out_hw, opts, name="seg_bce_upsample_loss", conf=None, zthr=0.0, C=1, expect=0):
    N, _, H, W = shape
    Ho, Wo = out_hw
    nwork = query("seg_bce_workspace_floats", N * Ho * Wo)
    work, stats = guarded(nwork), guarded(8)
    args = [lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, opts["pos_weight"], opts["bce"], opts["dice"],
            opts["focal_gamma"], opts["dice_smooth"], work.data_ptr(), stats.data_ptr()]
    if conf is not None:
        args += [zthr, conf.data_ptr()]
    rc = getattr(lib(), name)(*args, S())
    assert rc == expect, (name, rc)
    assert guard_ok(work, nwork) and guard_ok(stats, 8), name
    if expect:
        assert torch.all(work == SENTINEL) and torch.all(stats == SENTINEL)
    return stats[:8]


def run_grad(lg, ld, shape, yg, out_hw, stats, opts, name="seg_bce_upsample_grad", g=G, C=1, expect=0):
    N, _, H, W = shape
    Ho, Wo = out_hw
    gout = torch.tensor([g], device=DEV)
    dhigh = guarded(N * Ho * Wo, fill=5.0)
    rc = getattr(lib(), name)(lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, opts["pos_weight"],
                              opts["bce"], opts["dice"], opts["focal_gamma"], gout.data_ptr(), stats.data_ptr(),
                              dhigh.data_ptr(), S())
    assert rc == expect, (name, rc)
    assert guard_ok(dhigh, N * Ho * Wo, 5.0), name
    if expect:
        assert torch.all(dhigh == 5.0)
    return dhigh[:N * Ho * Wo]


def low_grad(dhigh, shape, out_hw, ac=2, io=False):
    """The low-resolution gradient [N, 1, H, W] on the CPU: seg_upsample_bwd on the fp32 plane."""
    N, _, H, W = shape
    Ho, Wo = out_hw
    if H == 1 and W == 1:  # every tap weight is 1 (seg_upsample_bwd's tap search divides by the zero scale)
        return dhigh.reshape(N, -1).sum(1).reshape(N, 1, 1, 1).double().cpu()
    dlow = torch.empty(N * H * W, 4, device=DEV, dtype=BF if io else torch.float32)
    call("seg_upsample_bwd_bf16io" if io else "seg_upsample_bwd", dhigh.data_ptr(), 0, 1, N, Ho, Wo, 1,
         dlow.data_ptr(), 4, H, W, ac, 0, S())
    return dlow[:, 0].double().reshape(N, 1, H, W).cpu()


def check_against_reference(ref, stats, got, record=None, tag=None, abs_tol=0.0):
    """The stats slots, the Dice coefficients, the loss terms and the low-resolution gradient."""
    o = stats.cpu().double().tolist()
    tag = (tag, o, ref["loss"], ref["F"], ref["Dice"])
    assert o[1] == o[3] == ref["nvalid"] and o[2] == 0, tag
    grad = ref["grad"]
    finite = bool(torch.isfinite(grad).all())
    errs = {k: (abs(o[slot] - ref[k]) / max(abs(ref[k]), 1e-30)) for k, slot in (("loss", 0), ("F", 4), ("Dice", 5))
            if ref[k] is not None and ref[k] == ref[k]}
    e_grad = rel(got, grad) if finite and float(grad.abs().max()) > 0.0 else 0.0
    b_loss = b_grad = TOL
    if max(list(errs.values()) + [0.0]) > TOL or e_grad >= TOL:
        f_loss, f_grad = fp32_bounds(ref)
        b_loss, b_grad = max(TOL, f_loss), max(TOL, f_grad)
        if record is not None:
            record(case=str(tag[0]), errs=errs, grad_err=e_grad, loss_bound=b_loss, grad_bound=b_grad)
    print(tag[0], "errors", errs, "grad", e_grad, "bounds", b_loss, b_grad)
    for k, slot in (("loss", 0), ("F", 4), ("Dice", 5)):
        if ref[k] is None:
            continue
        if ref[k] != ref[k]:  # 0/0, as aten
            assert o[slot] != o[slot], (k, tag)
        else:
            assert abs(o[slot] - ref[k]) <= b_loss * abs(ref[k]) + 1e-7, (k, tag)
    for k, slot in (("a", 6), ("b", 7)):
        assert abs(o[slot] - ref[k]) <= TOL * abs(ref[k]), (k, tag)
    if not finite:
        assert not torch.isfinite(got).all(), tag
    elif float(grad.abs().max()) == 0.0:
        assert float(got.abs().max()) <= 1e-7, tag
    else:
        assert float((got.double() - grad).norm()) <= b_grad * float(grad.norm()) + abs_tol, (tag, e_grad)
    return e_grad


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("shape,out_hw", SHAPES, ids=[IDS(s) for s in SHAPES])
def test_loss_and_gradient_against_fp64(shape, out_hw, ld, record):
    low, y = case(shape, out_hw)
    lg, yg = rows(low, ld), y.to(DEV)
    ignored = (y == -100).reshape(-1).to(DEV)
    assert bool(ignored.any())
    for name, opts in CASES.items():
        stats = run_loss(lg, ld, shape, yg, out_hw, opts)
        dhigh = run_grad(lg, ld, shape, yg, out_hw, stats, opts)
        assert torch.all(dhigh[ignored] == 0)  # exactly
        ref = reference(low, y, name, (shape, out_hw))
        e2 = check_against_reference(ref, stats, low_grad(dhigh, shape, out_hw), record, (name, shape, out_hw, ld))
        if (shape, out_hw) == BIG and name == "all" and ld == 4:
            # the transpose of the kernels' own blend (ac = 2) beside aten's tap weights (ac = 1): DESIGN.md's figures
            e1 = rel(low_grad(dhigh, shape, out_hw, ac=1), ref["grad"])
            record(case="BIG all: low-resolution gradient error by seg_upsample_bwd's ac", ac1=e1, ac2=e2)
            print("BIG all: gradient error ac=1", e1, "ac=2", e2)


@pytest.mark.parametrize("shape,out_hw", [SMALL[0], SMALL[4], BIG], ids=[IDS(s) for s in (SMALL[0], SMALL[4], BIG)])
def test_bf16io_twins_against_fp64_of_the_rounded_logits(shape, out_hw, record):
    """The twins read bf16 rows: the reference is fp64 over the same rounded values.  Their stats are bitwise the
    fp32 entry points' on the widened rows, and so is the gradient plane (fp32 in both maths)."""
    low, y = case(shape, out_hw)
    low = low.to(BF).float()
    lg16, lg32, yg = rows(low, 4, BF), rows(low, 4), y.to(DEV)
    for name, opts in CASES.items():
        st16 = run_loss(lg16, 4, shape, yg, out_hw, opts, "seg_bce_upsample_loss_bf16io")
        st32 = run_loss(lg32, 4, shape, yg, out_hw, opts)
        assert torch.equal(st16.view(torch.int32), st32.view(torch.int32))
        d16 = run_grad(lg16, 4, shape, yg, out_hw, st16, opts, "seg_bce_upsample_grad_bf16io")
        d32 = run_grad(lg32, 4, shape, yg, out_hw, st32, opts)
        assert d16.dtype == torch.float32 and torch.equal(d16.view(torch.int32), d32.view(torch.int32))
        conf16, conf32 = guarded(4, torch.int64, 0), guarded(4, torch.int64, 0)
        e16 = run_loss(lg16, 4, shape, yg, out_hw, opts, "seg_bce_upsample_eval_bf16io", conf16, logit_threshold(0.3))
        run_loss(lg32, 4, shape, yg, out_hw, opts, "seg_bce_upsample_eval", conf32, logit_threshold(0.3))
        assert torch.equal(e16.view(torch.int32), st16.view(torch.int32)) and torch.equal(conf16, conf32)
        ref = reference(low, y, name, (shape, out_hw, "bf16"))
        check_against_reference(ref, st16, low_grad(d16, shape, out_hw), record, (name, shape, out_hw, "bf16io"))


def test_saturated_logits_stay_finite(record):
    """Logits x 30 (|z| up to ~150): exp(-|z|) underflows, 1 - pt is 0 on the pixels that are right -- everything is
    finite and within tolerance."""
    shape, out_hw = SMALL[0]
    low, y = case(shape, out_hw, 30.0)
    assert float(low.abs().max()) > 100
    lg, yg = rows(low), y.to(DEV)
    for name, opts in CASES.items():
        ref = reference(low, y, name, (shape, out_hw, "x30"))
        assert torch.isfinite(torch.tensor(ref["loss"])) and torch.isfinite(ref["grad"]).all()
        stats = run_loss(lg, 4, shape, yg, out_hw, opts)
        dhigh = run_grad(lg, 4, shape, yg, out_hw, stats, opts)
        assert torch.isfinite(stats).all() and torch.isfinite(dhigh).all()
        check_against_reference(ref, stats, low_grad(dhigh, shape, out_hw), record, (name, "x30"))


@pytest.mark.parametrize("shape,out_hw", [SMALL[0], BIG], ids=["small", "big"])
def test_two_calls_agree_bitwise(shape, out_hw):
    low, y = case(shape, out_hw)
    lg, yg = rows(low), y.to(DEV)
    opts = CASES["all"]
    runs = []
    for _ in range(2):
        stats = run_loss(lg, 4, shape, yg, out_hw, opts)
        runs.append((stats, run_grad(lg, 4, shape, yg, out_hw, stats, opts)))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def matrix64(z64, y, zthr, ignore=-100):
    valid = y != ignore
    pred = (z64[:, 0] > zthr)
    return torch.bincount(y[valid] * 2 + pred[valid].long(), minlength=4).reshape(2, 2)


@pytest.mark.parametrize("shape,out_hw", SHAPES, ids=[IDS(s) for s in SHAPES])
def test_eval_matrix_and_stats(shape, out_hw):
    """_eval: the loss call's stats, bitwise, and confusion[t][z > zthr] away from the threshold; it adds to what the
    matrix holds, and writes nothing behind its four entries."""
    low, y = case(shape, out_hw)
    lg = rows(low)
    z64 = upsample64(low, out_hw)
    for thr in THRESHOLDS:
        zthr = logit_threshold(thr)
        close = (z64[:, 0] - zthr).abs() < MARGIN
        share = float(close.float().mean())
        print(shape, thr, f"left out (|z - zthr| < {MARGIN} in fp64): {int(close.sum())} of {close.numel()}")
        assert share <= MAX_LEFT_OUT
        yy = y.clone()
        yy[close] = -100
        yg = yy.to(DEV)
        want = matrix64(z64, yy, zthr)
        for name in ("bce", "all"):
            opts = CASES[name]
            conf = guarded(4, torch.int64, 0)
            conf[:4] = torch.tensor([3, 1, 4, 1], device=DEV)  # accumulation into a non-zero matrix
            o_eval = run_loss(lg, 4, shape, yg, out_hw, opts, "seg_bce_upsample_eval", conf, zthr)
            o_loss = run_loss(lg, 4, shape, yg, out_hw, opts)
            assert torch.equal(o_eval.view(torch.int32), o_loss.view(torch.int32))
            assert guard_ok(conf, 4, 0)
            assert torch.equal(conf[:4].cpu().reshape(2, 2) - torch.tensor([[3, 1], [4, 1]]), want), (thr, name)
            assert int(want.sum()) == int(o_eval[1].item())
    if (shape, out_hw) != SMALL[3]:
        assert not torch.equal(matrix64(z64, y, logit_threshold(0.3)), matrix64(z64, y, logit_threshold(0.9)))


def test_exact_ties_are_background():
    """(5, 9) -> (9, 17): tap weights 0 and 0.5, low logits from {-2, 0, 2} -- every z is exact in fp32, many are
    exactly 0 = zthr(0.5), and the strict comparison bins all of them as background."""
    shape, out_hw = (2, 1, 5, 9), (9, 17)
    low = (torch.randint(0, 3, shape, generator=torch.Generator().manual_seed(4)) * 2 - 2).float()
    y = torch.randint(0, 2, (2, *out_hw), generator=torch.Generator().manual_seed(5))
    y[0, :2] = -100
    z64 = upsample64(low, out_hw)
    ties = (z64[:, 0] == 0) & (y != -100)
    assert int(ties.sum()) * 10 >= y.numel()
    assert logit_threshold(0.5) == 0.0
    for ld in (4, 8):
        conf = guarded(4, torch.int64, 0)
        run_loss(rows(low, ld), ld, shape, y.to(DEV), out_hw, CASES["bce"], "seg_bce_upsample_eval", conf, 0.0)
        got = conf[:4].cpu().reshape(2, 2)
        assert torch.equal(got, matrix64(z64, y, 0.0))
        assert int(got[:, 1].sum()) == int(((z64[:, 0] > 0) & (y != -100)).sum())
        # with the ties ignored instead, the background column loses exactly them
        y2 = y.clone()
        y2[ties] = -100
        conf2 = guarded(4, torch.int64, 0)
        run_loss(rows(low, ld), ld, shape, y2.to(DEV), out_hw, CASES["bce"], "seg_bce_upsample_eval", conf2, 0.0)
        diff = got - conf2[:4].cpu().reshape(2, 2)
        assert torch.equal(diff[:, 1], torch.zeros(2, dtype=torch.int64)) and int(diff[:, 0].sum()) == int(ties.sum())


@pytest.mark.parametrize("bad", [2, -1])
def test_out_of_range_label(bad):
    shape, out_hw = SMALL[1]
    low, y = case(shape, out_hw)
    y = y.clone()
    y[0, 5, 2] = bad
    lg, yg = rows(low), y.to(DEV)
    nvalid = int((y != -100).sum()) - 1
    z64 = upsample64(low, out_hw)
    yy = y.clone()
    yy[0, 5, 2] = -100
    for opts in CASES.values():
        conf = guarded(4, torch.int64, 0)
        stats = run_loss(lg, 4, shape, yg, out_hw, opts, "seg_bce_upsample_eval", conf, 0.0)
        assert stats[2].item() == 1 and torch.isnan(stats[0]) and stats[1].item() == stats[3].item() == nvalid
        assert torch.equal(conf[:4].cpu().reshape(2, 2), matrix64(z64, yy, 0.0))  # the bad label is in no bin
        dhigh = run_grad(lg, 4, shape, yg, out_hw, stats, opts, g=1.0)
        valid = ((y == 0) | (y == 1)).reshape(-1).to(DEV)
        assert torch.isnan(dhigh[valid]).all() and torch.all(dhigh[~valid] == 0)


def test_invalid_arguments_write_nothing():
    shape, out_hw = SMALL[0]
    low, y = case(shape, out_hw)
    lg, yg = rows(low, 8), y.to(DEV)
    opts = CASES["all"]
    good = run_loss(lg, 8, shape, yg, out_hw, opts)
    for kw in (dict(C=2), dict(ld=6), dict(opts=dict(opts, pos_weight=0.0)), dict(opts=dict(opts, pos_weight=-1.0))):
        o = kw.get("opts", opts)
        ld = kw.get("ld", 8)
        C = kw.get("C", 1)
        conf = guarded(4, torch.int64, 0)
        run_loss(lg, ld, shape, yg, out_hw, o, C=C, expect=1)
        run_loss(lg, ld, shape, yg, out_hw, o, "seg_bce_upsample_eval", conf, 0.0, C=C, expect=1)
        run_loss(lg.to(BF), ld, shape, yg, out_hw, o, "seg_bce_upsample_loss_bf16io", C=C, expect=1)
        assert torch.all(conf == 0)
        run_grad(lg, ld, shape, yg, out_hw, good, o, C=C, expect=1)
        run_grad(lg.to(BF), ld, shape, yg, out_hw, good, o, "seg_bce_upsample_grad_bf16io", C=C, expect=1)


# ---- seg_threshold_nearest ----

@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("fhw", [(36, 64), (37, 61)], ids=["36x64", "37x61"])
def test_threshold_nearest(fhw, thr):
    """(1, 1, 8, 16) low logits, a (32, 64) model grid; the reference is seg_upsample_to_nchw's fp32 logits,
    thresholded and mapped to the frame by the suite's INTER_NEAREST reference (oracle/cvresize.py)."""
    N, H, W, Hm, Wm = 1, 8, 16, 32, 64
    Hf, Wf = fhw
    low = torch.randn(N, 1, H, W, generator=torch.Generator().manual_seed(1)) * 2
    low[0, 0, 3, 5] = float("nan")
    lg = rows(low, 8)
    z = torch.empty(N, 1, Hm, Wm, device=DEV)
    call("seg_upsample_to_nchw", lg.data_ptr(), 8, N, H, W, 1, z.data_ptr(), Hm, Wm, 1, S())
    zthr = logit_threshold(thr)
    mask = guarded(Hf * Wf, torch.uint8, 9)
    call("seg_threshold_nearest", lg.data_ptr(), 8, N, H, W, Hm, Wm, zthr, mask.data_ptr(), Hf, Wf, S())
    assert guard_ok(mask, Hf * Wf, 9)
    got = mask[:Hf * Wf].cpu().numpy().reshape(Hf, Wf)
    assert set(np.unique(got)) <= {0, 1} and got.any() and not got.all()
    zc = z[0, 0].cpu().numpy().astype(np.float64)
    want = cvresize.resize_nearest((zc > zthr).astype(np.uint8), (Wf, Hf))
    nan = cvresize.resize_nearest(np.isnan(zc), (Wf, Hf))
    close = cvresize.resize_nearest(np.abs(zc - zthr) < MARGIN, (Wf, Hf))
    print(f"left out (|z - zthr| < {MARGIN}): {int(close.sum())} of {close.size}; NaN pixels {int(nan.sum())}")
    assert close.mean() <= MAX_LEFT_OUT
    assert nan.any() and not got[nan].any()  # a NaN logit gives 0
    assert np.array_equal(got[~close], want[~close])
