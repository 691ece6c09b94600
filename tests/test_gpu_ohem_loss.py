"""GPU: the online-hard-example-mining loss kernels (csrc/loss.hip: seg_ohem_upsample_loss / _grad / _eval and their
_bf16io twins), called through the C ABI.  Two kinds of check, kept apart:

Values -- against seg_amd.losses.ohem_loss_terms in fp64 on the CPU over F.interpolate(..., align_corners=True) of the
same low-resolution logits (the bf16-rounded ones for the twins), upstream gradient 0.7.  Loss and low-resolution
gradient: the tolerance tests/test_gpu_seg_loss.py takes from tests/test_gpu_loss_options.py, 1e-5 relative (+1e-7)
on the loss and 1e-5 relative norm on the gradient.  So that rounding cannot move a pixel across the cut, every value
case first asserts, on the reference alone, that no valid pixel's fp64 loss other than the k-th largest itself lies
within 1e-4 of the cut (ten times the tolerance at losses up to 10); the seeds below were picked on the CPU to satisfy
it, and a case that does not fails.  The per-pixel buffer (the first N*Ho*Wo floats of the workspace) is held to an
absolute bound from the number formats: 2^-20 (1 + max |z|) for the blend, exp, log and the two sums (a few fp32 ulps
of the largest magnitude), plus 2^-23 (max(H, W) + 1) times the largest difference between neighbouring low-resolution
logits -- the fp32 source coordinate scale * dst carries the relative error 2^-24 of `scale`, which moves the tap
weights by up to 2^-24 max(H, W) in each direction.  The bf16io gradient twin writes the full-resolution gradient in
fp32 (NCHW); it must equal, element for element, the fp32 kernel's on the widened logits, and that gradient is held to
the 1e-5 (the low-resolution gradient the twin's consumer then stores in bf16 is another kernel's rounding).

Selection, exact -- lambda, cut, #kept and K are recomputed on the host from the kernel's OWN per-pixel buffer with
np.partition; stats[4], stats[5], #valid and #out-of-range match exactly and the set of non-zero gradient rows is K.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from seg_amd._lib import call, lib, query
from seg_amd.losses import ohem_loss_terms

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
G = 0.7  # the upstream gradient
TOL = 1e-5
GAP = 1e-4
THRESH = 0.7
TOPK = 1e-30  # a thresh no loss reaches (tau = 69): the floor alone selects

BIG = (1, 4, 384, 352)  # 540 672 output pixels > 2048 blocks x 256: the grid-stride loops run more than once
SMALL = [(2, 3, 12, 20), (2, 10, 12, 20), (2, 32, 12, 20), (1, 10, 5, 7)]  # 1920 pixels: 8 blocks, no multiple of 256


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


def weights(C):
    return torch.rand(C, generator=torch.Generator().manual_seed(3)) * 3 + 0.05


# ---------------------------------------------------------------------------------------------------------- inputs
_CASES = {}


def case(shape, seed, scale=2.0, margin=6.0):
    """(low-resolution logits, labels): random logits leave almost every pixel hard, so the label's logit of about
    half the low-resolution pixels gets a margin -- the labels are a low-resolution class map doubled, so the four
    taps of a pixel mostly agree on its class.  The first two rows of image 0 are ignored."""
    key = (shape, seed, scale, margin)
    if key not in _CASES:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(seed)
        low = torch.randn(N, C, H, W, generator=g) * scale
        yl = torch.randint(0, C, (N, H, W), generator=g)
        easy = (torch.rand(N, H, W, generator=g) < 0.5).float() * margin * (scale / 2.0)
        low.scatter_add_(1, yl.unsqueeze(1), easy.unsqueeze(1))
        y = yl.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
        y[0, :2] = -100
        _CASES[key] = (low, y)
    return _CASES[key]


def big_case(seed):
    """BIG: four vertical stripes of one class each, eight horizontal bands alternately easy (the label's logit + 5)
    and hard (- 3) over small noise, so the losses form two groups (about 0.02 and about 4) with only the pixels of
    the band and stripe borders between them, and a cut can lie in a gap at 540 672 pixels."""
    key = ("big", seed)
    if key not in _CASES:
        N, C, H, W = BIG
        g = torch.Generator().manual_seed(seed)
        low = torch.randn(N, C, H, W, generator=g) * 0.3
        yl = (torch.arange(W) // (W // C)).clamp(max=C - 1).view(1, 1, W).expand(N, H, W).contiguous()
        band = ((torch.arange(H) // (H // 8)) % 2 == 0).float().view(1, H, 1).expand(N, H, W)
        low.scatter_add_(1, yl.unsqueeze(1), (band * 8.0 - 3.0).unsqueeze(1).contiguous())
        y = yl.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
        y[0, :2] = -100
        _CASES[key] = (low, y)
    return _CASES[key]


# the seeds satisfy the gap precondition for every mode of test_values (searched on the CPU, fp32 and bf16-rounded)
SEEDS = {((2, 3, 12, 20), "f32"): 4, ((2, 10, 12, 20), "f32"): 1, ((2, 32, 12, 20), "f32"): 1,
         ((1, 10, 5, 7), "f32"): 2, (BIG, "f32"): 4,
         ((2, 3, 12, 20), "bf16"): 1, ((2, 10, 12, 20), "bf16"): 1, ((2, 32, 12, 20), "bf16"): 1,
         ((1, 10, 5, 7), "bf16"): 2, (BIG, "bf16"): 7}


def value_inputs(shape, io):
    seed = SEEDS[(shape, "bf16" if io else "f32")]
    low, y = big_case(seed) if shape == BIG else case(shape, seed)
    if io:  # what the twin reads
        low = _CASES.setdefault(("bf16", shape, seed), low.to(BF).float())
    return low, y


def modes(low, y):
    """{name: (thresh, k)} of a value case, from the fp64 losses: threshold mode (the count above tau = 0.357 reaches
    k), and top-k mode with tau = 3.0 and the floor where the losses cross 1 -- a region thin enough for the gap.  (A
    floor of |V| or more puts lambda on the smallest loss, among easy pixels far closer together than the gap: those
    floors are selection cases below, where nothing is compared across roundings.)"""
    lv = pixel_losses(low, y)[y != -100]
    above = int((lv > -math.log(THRESH)).sum())
    return {"threshold": (THRESH, max(above // 3, 1)), "floor": (0.05, int((lv > 1.0).sum()))}


_L64 = {}


def pixel_losses(low, y):
    key = (id(low), id(y))
    if key not in _L64:
        z = F.interpolate(low.double(), size=tuple(y.shape[1:]), mode="bilinear", align_corners=True)
        yy = torch.where(y == -100, torch.zeros_like(y), y)
        _L64[key] = (-torch.log_softmax(z, 1).gather(1, yy.unsqueeze(1)).squeeze(1), low, y)
    return _L64[key][0]


_REFS = {}


def reference(low, y, w, thresh, k):
    """fp64 CPU: dict(loss, grad, kept, cut, l, D, nvalid).  Made once per case and shared; asserts the gap."""
    key = (id(low), id(y), w is None, thresh, k)
    if key not in _REFS:
        lr = low.double().clone().requires_grad_(True)
        z = F.interpolate(lr, size=tuple(y.shape[1:]), mode="bilinear", align_corners=True)
        loss, kept, cut = ohem_loss_terms(z, y, thresh, k, None if w is None else w.double())
        loss.backward(torch.tensor(G, dtype=torch.float64))
        valid = y != -100
        l = pixel_losses(low, y)
        d = (l[valid] - cut).abs().sort().values
        tau = -math.log(thresh)
        # the gap: no valid pixel's loss other than the k-th largest itself (distance 0 in top-k mode) near the cut
        nearest = float(d[1] if float(cut) < tau else d[0])
        assert nearest > GAP, f"precondition: a valid pixel's fp64 loss lies {nearest:.3e} from the cut {float(cut)}"
        wy = torch.ones(low.shape[1], dtype=torch.float64) if w is None else w.double()
        _REFS[key] = dict(loss=float(loss.detach()), grad=lr.grad, kept=kept, cut=float(cut), l=l,
                          D=float(wy[y[kept]].sum()), nvalid=int(valid.sum()), keep=(low, y, w))
    return _REFS[key]


# -------------------------------------------------------------------------------------------------------- launches
def run_loss(lg, ld, N, H, W, C, yg, w, thresh, k, io=False, conf=None, work=None):
    """(out6, work): a fresh workspace is filled with a large value first -- the entry point clears what it needs."""
    Ho, Wo = 2 * H, 2 * W
    out6 = torch.full((6,), -7.0, device=DEV)
    if work is None:
        work = torch.full((query("seg_ohem_workspace_floats", N * Ho * Wo),), 3e38, device=DEV)
    name = "seg_ohem_upsample_" + ("loss" if conf is None else "eval") + ("_bf16io" if io else "")
    args = [lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, w.data_ptr() if w is not None else None,
            -math.log(thresh), k, work.data_ptr(), out6.data_ptr()]
    if conf is not None:
        args.append(conf.data_ptr())
    call(name, *args, S())
    return out6, work


def run_grad(lg, ld, N, H, W, C, yg, w, thresh, work, stats, io=False, ldh=None, g=G):
    """The full-resolution gradient as fp32 rows [N*Ho*Wo, ldh].  The bf16io twin writes fp32 NCHW [N, C, Ho, Wo]
    (and nothing around it: the buffer has 8 floats more, checked here); its planes are laid out as rows, the pad
    columns zero, so that every check reads both forms alike."""
    Ho, Wo = 2 * H, 2 * W
    ldh = ldh or r4(C)
    gout = torch.tensor([g], device=DEV)
    wp = w.data_ptr() if w is not None else None
    if io:
        flat = torch.full((N * C * Ho * Wo + 8,), 5.0, device=DEV)
        call("seg_ohem_upsample_grad_bf16io", lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, wp,
             -math.log(thresh), work.data_ptr(), gout.data_ptr(), stats.data_ptr(), flat.data_ptr(), S())
        assert torch.all(flat[-8:] == 5.0)
        dhigh = torch.zeros((N * Ho * Wo, ldh), device=DEV)
        dhigh[:, :C] = flat[:-8].view(N, C, Ho * Wo).permute(0, 2, 1).reshape(-1, C)
        return dhigh
    dhigh = torch.full((N * Ho * Wo, ldh), 5.0, device=DEV)
    call("seg_ohem_upsample_grad", lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, wp, -math.log(thresh),
         work.data_ptr(), gout.data_ptr(), stats.data_ptr(), dhigh.data_ptr(), ldh, S())
    return dhigh


def low_grad(dhigh, N, C, H, W, ldh=None):
    ldh = ldh or r4(C)
    dlow = torch.empty(N * H * W, r4(C), device=DEV)
    call("seg_upsample_bwd", dhigh.data_ptr(), ldh, 0, N, 2 * H, 2 * W, C, dlow.data_ptr(), r4(C), H, W, 1, 0, S())
    return dlow


def buffer_bound(low):
    """The absolute bound on a per-pixel loss (module docstring)."""
    H, W = low.shape[2:]
    step = max(float((low[:, :, 1:] - low[:, :, :-1]).abs().max()), float((low[..., 1:] - low[..., :-1]).abs().max()))
    return 2.0 ** -20 * (1.0 + float(low.abs().max())) + 2.0 ** -23 * (max(H, W) + 1) * step


def check_selection(work, stats, dhigh, y, C, thresh, k, w=None, nbad=0, underflow=False):
    """The exact checks, from the kernel's own per-pixel buffer.  Returns (K as a bool array, lambda, buffer).
    underflow: logits so far apart that a kept pixel's whole gradient row may round to zero (every other class's
    softmax underflows and the label's is exactly 1); the rows of the kept pixels with a loss above 1e-6 still may
    not, and no row outside K may be non-zero."""
    pixels = y.numel()
    buf = work[:pixels].cpu().numpy()
    yy = y.reshape(-1).numpy()
    valid = (yy != -100) & (yy >= 0) & (yy < C)
    assert np.all(buf[~valid] == -1.0) and np.all(buf[valid] >= 0.0)
    lv = buf[valid]
    nv = lv.size
    tau = np.float32(-math.log(thresh))
    st = stats.cpu().numpy()
    assert st[3] == nv and st[2] == nbad == int(((yy != -100) & ~valid).sum())
    if nv == 0:
        assert st[4] == 0 and st[5] == tau and np.isnan(st[0])
        return np.zeros(pixels, bool), None, buf
    ke = min(k, nv)
    lam = np.partition(lv, nv - ke)[nv - ke]  # the ke-th largest
    K = valid & ((buf > tau) | (buf >= lam))
    assert st[4] == K.sum(), (st, K.sum(), lam, tau)
    assert st[5] == min(tau, lam), (st, lam, tau)
    if dhigh is not None and nbad == 0:
        rows = (dhigh[:, :C].float() != 0).any(1).cpu().numpy()
        if underflow:
            assert not (rows & ~K).any() and rows[K & (buf > 1e-6)].all(), (rows.sum(), K.sum())
        else:
            assert np.array_equal(rows, K), (rows.sum(), K.sum())
        assert bool(torch.all(dhigh[:, C:r4(C)].float() == 0))
    if nbad == 0:
        wy = np.ones(C) if w is None else w.double().numpy()
        D = wy[yy[K]].sum()
        assert abs(st[1] - D) <= 1e-6 * D, (st, D)
        want = (wy[yy[K]] * buf[K].astype(np.float64)).sum() / D
        assert abs(st[0] - want) <= 1e-6 * abs(want) + 1e-7, (st, want)
    return K, lam, buf


# ---------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
@pytest.mark.parametrize("shape,ld", [(s, None) for s in SMALL] + [((2, 10, 12, 20), 16), (BIG, None)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"ld{v}")
def test_values(shape, ld, io):
    N, C, H, W = shape
    ld = ld or r4(C)
    low, y = value_inputs(shape, io)
    lg32, yg = nhwc(low, ld), y.to(DEV)
    lg = lg32.to(BF) if io else lg32
    bound = buffer_bound(low)
    for use_w in (False, True):
        w = weights(C) if use_w else None
        wg = None if w is None else w.to(DEV)
        for name, (thresh, k) in modes(low, y).items():
            ref = reference(low, y, w, thresh, k)
            tag = (shape, ld, io, use_w, name, thresh, k)
            out6, work = run_loss(lg, ld, N, H, W, C, yg, wg, thresh, k, io)
            buf = work[:y.numel()].cpu().double().reshape(y.shape)
            valid = y != -100
            e_buf = float((buf - ref["l"])[valid].abs().max())
            o = out6.cpu().double().tolist()
            e_loss = abs(o[0] - ref["loss"]) / abs(ref["loss"])
            o32, work32 = run_loss(lg32, ld, N, H, W, C, yg, wg, thresh, k) if io else (out6, work)
            d32 = run_grad(lg32, ld, N, H, W, C, yg, wg, thresh, work32, o32)
            e_grad = rel(from_nhwc(low_grad(d32, N, C, H, W), N, C, H, W), ref["grad"])
            print(tag, "buffer", e_buf, "bound", bound, "loss", e_loss, "grad", e_grad, "stats", o, "ref cut",
                  ref["cut"])
            assert torch.all(buf[~valid] == -1.0) and e_buf <= bound, tag
            assert o[3] == ref["nvalid"] and o[2] == 0 and o[4] == int(ref["kept"].sum()), tag
            assert abs(o[5] - ref["cut"]) <= bound, tag  # one pixel's loss (or tau as a float): the buffer's bound
            assert abs(o[1] - ref["D"]) <= TOL * ref["D"] + 1e-7, tag
            assert abs(o[0] - ref["loss"]) <= TOL * abs(ref["loss"]) + 1e-7, tag
            kept = (d32[:, :C] != 0).any(1).cpu().reshape(y.shape)
            assert torch.equal(kept, ref["kept"]), tag
            assert e_grad <= TOL, tag
            if io:  # the twin's gradient (fp32 NCHW): the fp32 kernel's on the same values, element for element
                d16 = run_grad(lg, ld, N, H, W, C, yg, wg, thresh, work, out6, io=True)
                assert torch.equal(d16[:, :C], d32[:, :C]), tag
                assert torch.equal(o32.view(torch.int32), out6.view(torch.int32)), tag


# ------------------------------------------------------------------------------------------------------- selection
SEL = (2, 10, 12, 20)


def _run_sel(low, y, thresh, k, w=None, ld=None, io=False):
    N, C, H, W = low.shape
    ld = ld or r4(C)
    lg, yg = nhwc(low, ld, BF if io else torch.float32), y.to(DEV)
    wg = None if w is None else w.to(DEV)
    out6, work = run_loss(lg, ld, N, H, W, C, yg, wg, thresh, k, io)
    dhigh = run_grad(lg, ld, N, H, W, C, yg, wg, thresh, work, out6, io)
    return out6, work, dhigh


@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
@pytest.mark.parametrize("shape", SMALL + [BIG], ids=lambda s: "x".join(map(str, s)))
def test_selection_modes(shape, io):
    N, C, H, W = shape
    low, y = big_case(5) if shape == BIG else case(shape, 5)
    nv = int((y != -100).sum())
    seen = set()
    for thresh, k in ((THRESH, 1), (THRESH, nv // 8), (THRESH, nv - nv // 4), (TOPK, 1), (TOPK, nv // 2), (TOPK, nv),
                      (TOPK, nv + 1000), (0.05, nv // 2)):
        out6, work, dhigh = _run_sel(low, y, thresh, k, weights(C), io=io)
        K, lam, buf = check_selection(work, out6, dhigh, y, C, thresh, k, weights(C))
        mode = "threshold" if (buf > np.float32(-math.log(thresh))).sum() >= min(k, nv) else "topk"
        seen.add(mode)
        if thresh == TOPK:
            assert mode == "topk" and K.sum() >= min(k, nv)
        if (thresh, k) == (TOPK, 1):
            assert K.sum() == 1 and buf[K][0] == buf.max()
        if k >= nv:
            assert K.sum() == nv
    assert seen == {"threshold", "topk"}


def test_lambda_in_different_top_level_bins():
    """The logits scaled: at 0.01 every loss is log C to within a few hundredths and the top digit cannot tell them
    apart (the two lower digits decide); at 30 the losses spread over many binades."""
    bins = {}
    for scale in (0.01, 0.25, 2.0, 30.0):
        low, y = case(SEL, 7, scale=scale)
        nv = int((y != -100).sum())
        for k in (nv // 10, nv // 2, nv - 3):
            out6, work, dhigh = _run_sel(low, y, TOPK, k)
            K, lam, _ = check_selection(work, out6, dhigh, y, SEL[1], TOPK, k, underflow=scale > 2.0)
            assert K.sum() == k or scale > 2.0  # random logits: no ties (but saturated zeros at scale 30)
            bins.setdefault(scale, set()).add(int(np.float32(lam).view(np.uint32)) >> 20)
    print("top-level bins of lambda", bins)
    assert len(bins[0.01]) == 1 and len(bins[30.0]) == 3 and len(set().union(*bins.values())) >= 6, bins


def test_saturated_pixels_with_a_loss_of_exactly_zero():
    """The top half of image 1 has one class 40 above the rest and carries its label: se is exactly 1 and l_p exactly
    0 there.  A floor that reaches into the zeros keeps every one of them (lambda = 0)."""
    low, y = case(SEL, 7)
    low, y = low.clone(), y.clone()
    N, C, H, W = SEL
    low[1, :, :H // 2] = 0.0
    low[1, 4, :H // 2] = 40.0
    y[1, :H - 2] = 4  # rows whose two row taps both lie in the saturated half
    nv = int((y != -100).sum())
    out6, work, _ = _run_sel(low, y, TOPK, 1)
    buf = work[:y.numel()].cpu().numpy()
    zeros = int((buf == 0.0).sum())
    assert zeros >= (H - 2) * 2 * W
    for k in (nv - zeros + 5, nv - 1):
        out6, work, dhigh = _run_sel(low, y, TOPK, k)
        K, lam, _ = check_selection(work, out6, dhigh, y, C, TOPK, k)
        assert lam == 0.0 and K.sum() == nv and out6[5].item() == 0.0 and out6[4].item() == nv
    out6, work, dhigh = _run_sel(low, y, TOPK, nv - zeros)  # the floor stops just above them: none is kept
    K, lam, _ = check_selection(work, out6, dhigh, y, C, TOPK, nv - zeros)
    assert lam > 0.0 and K.sum() == nv - zeros


def test_a_tie_group_at_lambda_is_kept_whole():
    """Piecewise-constant low-resolution logits (powers of two, so the blend of equal taps is exact up to the tap
    weights' sum): many pixels share one l_p.  The floor is put inside the largest group of equal losses."""
    N, C, H, W = SEL
    g = torch.Generator().manual_seed(11)
    blocks = torch.randint(0, 5, (N, C, 3, 4), generator=g).float()
    low = (2.0 ** blocks).repeat_interleave(H // 3, 2).repeat_interleave(W // 4, 3).contiguous()
    y = torch.randint(0, C, (N, 3, 4), generator=g).repeat_interleave(2 * H // 3, 1).repeat_interleave(2 * W // 4, 2)
    y = y.contiguous()
    y[0, :2] = -100
    out6, work, _ = _run_sel(low, y, TOPK, 1)
    buf = work[:y.numel()].cpu().numpy()
    vals, counts = np.unique(buf[buf >= 0], return_counts=True)
    i = int(np.argmax(counts))
    assert counts[i] >= 4, counts.max()
    bigger = int((buf > vals[i]).sum())
    for k in (bigger + 1, bigger + counts[i] // 2, bigger + counts[i]):
        out6, work, dhigh = _run_sel(low, y, TOPK, int(k))
        K, lam, _ = check_selection(work, out6, dhigh, y, C, TOPK, int(k))
        assert lam == vals[i] and K.sum() == bigger + counts[i]


@pytest.mark.parametrize("shape", [SEL, (2, 3, 12, 20), BIG], ids=lambda s: "x".join(map(str, s)))
def test_on_K_the_gradient_is_the_weighted_kernels(shape):
    """With K fixed the criterion is nn.CrossEntropyLoss(weight) on the labels with every pixel outside K ignored.
    The kernels keep that to the bit: D, the loss and every gradient row equal seg_cew_upsample_loss / _grad's on
    those labels (same recomputed logits, same expressions, the same order of the partial sums)."""
    N, C, H, W = shape
    Ho, Wo = 2 * H, 2 * W
    low, y = big_case(5) if shape == BIG else case(shape, 5)
    nv = int((y != -100).sum())
    lg, w = nhwc(low), weights(C).to(DEV)
    for thresh, k in ((THRESH, 10), (TOPK, nv // 2)):
        out6, work = run_loss(lg, r4(C), N, H, W, C, y.to(DEV), w, thresh, k)
        dhigh = run_grad(lg, r4(C), N, H, W, C, y.to(DEV), w, thresh, work, out6)
        K, _, _ = check_selection(work, out6, dhigh, y, C, thresh, k, weights(C))
        yk = torch.where(torch.from_numpy(K).reshape(y.shape), y, torch.full_like(y, -100)).to(DEV)
        out4 = torch.full((4,), -7.0, device=DEV)
        cwork = torch.empty(query("seg_cew_workspace_floats", N * Ho * Wo), device=DEV)
        call("seg_cew_upsample_loss", lg.data_ptr(), r4(C), N, H, W, C, yk.data_ptr(), Ho, Wo, -100, w.data_ptr(), 0.0,
             0, cwork.data_ptr(), out4.data_ptr(), S())
        gout = torch.tensor([G], device=DEV)
        dcew = torch.full((N * Ho * Wo, r4(C)), 5.0, device=DEV)
        call("seg_cew_upsample_grad", lg.data_ptr(), r4(C), N, H, W, C, yk.data_ptr(), Ho, Wo, -100, w.data_ptr(), 0.0,
             gout.data_ptr(), out4.data_ptr(), dcew.data_ptr(), r4(C), S())
        print(shape, thresh, k, "OHEM", out6.tolist(), "weighted CE on K", out4.tolist())
        assert out4[1].item() == out6[1].item() and out4[3].item() == out6[4].item()
        assert out4[0].item() == out6[0].item()
        assert torch.equal(dcew, dhigh)


def test_class_weights_enter_the_mean_not_the_selection():
    low, y = case(SEL, 5)
    N, C, H, W = SEL
    nv = int((y != -100).sum())
    w = weights(C)
    w[3] = 0.0  # a class without weight is still selected, and adds nothing to D
    for thresh, k in ((THRESH, 10), (TOPK, nv // 2)):
        o_w, work_w, _ = _run_sel(low, y, thresh, k, w)
        o_1, work_1, _ = _run_sel(low, y, thresh, k, None)
        check_selection(work_w, o_w, None, y, C, thresh, k, w)
        assert torch.equal(o_w[2:], o_1[2:]) and torch.equal(work_w[:y.numel()], work_1[:y.numel()])
        assert o_w[1].item() != o_1[1].item() and o_1[1].item() == o_1[4].item()


def test_all_pixels_ignored():
    low, y = case(SEL, 5)
    y = torch.full_like(y, -100)
    out6, work, dhigh = _run_sel(low, y, THRESH, 100)
    check_selection(work, out6, None, y, SEL[1], THRESH, 100)
    assert torch.isnan(out6[0]) and out6[1].item() == 0 and torch.all(dhigh[:, :r4(SEL[1])] == 0)


@pytest.mark.parametrize("bad", [10, 255, -1])
def test_one_out_of_range_label(bad):
    low, y = case(SEL, 5)
    y = y.clone()
    y[1, 3, 4] = bad
    N, C, H, W = SEL
    for thresh, k in ((THRESH, 10), (TOPK, 500)):
        out6, work, dhigh = _run_sel(low, y, thresh, k, weights(C))
        check_selection(work, out6, None, y, C, thresh, k, nbad=1)
        assert out6[2].item() == 1 and torch.isnan(out6[0]) and out6[3].item() == (y != -100).sum().item() - 1
        assert torch.isnan(dhigh[:, :C]).any() and torch.all(dhigh[:, C:r4(C)] == 0)
        assert torch.all(dhigh[(1 * 2 * H + 3) * 2 * W + 4] == 0)  # the pixel itself: a zero row


def test_a_reused_workspace_is_cleared_by_every_call():
    """Two calls in a row on one workspace, with other labels and another floor: the second is bit for bit what a
    fresh workspace gives."""
    N, C, H, W = SEL
    low, y1 = case(SEL, 5)
    _, y2 = case(SEL, 6)
    lg, w = nhwc(low), weights(C).to(DEV)
    nv = int((y2 != -100).sum())
    for (t1, k1), (t2, k2) in (((TOPK, nv // 2), (TOPK, nv // 5)), ((TOPK, nv // 3), (THRESH, 7)),
                               ((THRESH, 7), (TOPK, nv - 9))):
        _, work = run_loss(lg, 12, N, H, W, C, y1.to(DEV), w, t1, k1)
        o_b, work = run_loss(lg, 12, N, H, W, C, y2.to(DEV), w, t2, k2, work=work)
        d_b = run_grad(lg, 12, N, H, W, C, y2.to(DEV), w, t2, work, o_b)
        o_f, fresh = run_loss(lg, 12, N, H, W, C, y2.to(DEV), w, t2, k2)
        d_f = run_grad(lg, 12, N, H, W, C, y2.to(DEV), w, t2, fresh, o_f)
        assert torch.equal(o_b.view(torch.int32), o_f.view(torch.int32))
        assert torch.equal(work[:y2.numel()].view(torch.int32), fresh[:y2.numel()].view(torch.int32))
        assert torch.equal(d_b.view(torch.int32), d_f.view(torch.int32))
        check_selection(work, o_b, d_b, y2, C, t2, k2, weights(C))


@pytest.mark.parametrize("shape", [SEL, (2, 3, 12, 20), (2, 32, 12, 20)], ids=lambda s: "x".join(map(str, s)))
def test_eval_is_the_loss_plus_the_plain_confusion_matrix(shape):
    N, C, H, W = shape
    Ho, Wo = 2 * H, 2 * W
    low, y = case(shape, 5)
    nv = int((y != -100).sum())
    ld = r4(C)
    for io in (False, True):
        lg, yg, wg = nhwc(low, ld, BF if io else torch.float32), y.to(DEV), weights(C).to(DEV)
        ref = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        out3 = torch.empty(3, device=DEV)
        cwork = torch.empty(query("seg_ce_workspace_floats", N * Ho * Wo), device=DEV)
        call("seg_ce_upsample_eval" + ("_bf16io" if io else ""), lg.data_ptr(), ld, N, H, W, C, yg.data_ptr(), Ho, Wo,
             -100, cwork.data_ptr(), out3.data_ptr(), ref.data_ptr(), S())
        assert int(ref.sum()) == nv
        for thresh, k in ((THRESH, 10), (TOPK, nv // 2)):
            conf = torch.zeros(C * C + 8, dtype=torch.int64, device=DEV)
            o_eval, w_eval = run_loss(lg, ld, N, H, W, C, yg, wg, thresh, k, io, conf)
            o_loss, w_loss = run_loss(lg, ld, N, H, W, C, yg, wg, thresh, k, io)
            assert torch.equal(o_eval.view(torch.int32), o_loss.view(torch.int32))
            assert torch.equal(w_eval[:y.numel()].view(torch.int32), w_loss[:y.numel()].view(torch.int32))
            assert o_eval[4].item() < nv  # the matrix is over all valid pixels, not over K
            assert torch.equal(conf[:C * C].reshape(C, C), ref) and torch.all(conf[C * C:] == 0)
            run_loss(lg, ld, N, H, W, C, yg, wg, thresh, k, io, conf)  # accumulates
            assert torch.equal(conf[:C * C].reshape(C, C), 2 * ref) and torch.all(conf[C * C:] == 0)


@pytest.mark.parametrize("shape", [SEL, BIG], ids=["small", "big"])
def test_two_calls_agree_bitwise(shape):
    N, C, H, W = shape
    low, y = big_case(5) if shape == BIG else case(shape, 5)
    nv = int((y != -100).sum())
    for thresh, k in ((THRESH, 10), (TOPK, nv // 2)):
        a = _run_sel(low, y, thresh, k, weights(C))
        b = _run_sel(low, y, thresh, k, weights(C))
        n = y.numel()
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert torch.equal(a[1][:n].view(torch.int32), b[1][:n].view(torch.int32))
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def test_row_strides():
    """ld = 16 for C = 10 (a channel slice of a wider buffer), and a dhigh row stride other than the logits'."""
    N, C, H, W = SEL
    low, y = case(SEL, 5)
    yg, w = y.to(DEV), weights(C).to(DEV)
    k = int((y != -100).sum()) // 2
    lg16, lg12 = nhwc(low, 16), nhwc(low, 12)
    o16, w16 = run_loss(lg16, 16, N, H, W, C, yg, w, TOPK, k)
    o12, w12 = run_loss(lg12, 12, N, H, W, C, yg, w, TOPK, k)
    assert torch.equal(o16, o12) and torch.equal(w16[:y.numel()], w12[:y.numel()])
    d12 = run_grad(lg12, 12, N, H, W, C, yg, w, TOPK, w12, o12)
    d16 = run_grad(lg16, 16, N, H, W, C, yg, w, TOPK, w16, o16, ldh=16)
    dmix = run_grad(lg12, 12, N, H, W, C, yg, w, TOPK, w12, o12, ldh=16)
    for d in (d16, dmix):
        assert torch.equal(d[:, :12], d12)
        assert torch.all(d[:, 12:] == 5.0)  # behind round4(C): not this kernel's to write


def test_bad_arguments_return_the_error_code_without_a_launch():
    N, C, H, W = 1, 10, 4, 6
    Ho, Wo = 2 * H, 2 * W
    low, y = case((N, C, H, W), 5)
    lg, yg = nhwc(low, 12), y.to(DEV)
    h = lib()
    pixels = N * Ho * Wo
    work = torch.full((query("seg_ohem_workspace_floats", pixels),), -3.0, device=DEV)
    out6 = torch.full((6,), -7.0, device=DEV)
    dhigh = torch.full((pixels, 12), 5.0, device=DEV)
    conf = torch.zeros(C * C, dtype=torch.int64, device=DEV)
    gout = torch.ones(1, device=DEV)
    ok = dict(ld=12, C=C, tau=0.35, k=5, ldh=12)
    for bad in (dict(C=0), dict(C=33), dict(ld=10), dict(ld=8), dict(k=0), dict(k=-4), dict(tau=-0.5),
                dict(tau=float("inf")), dict(tau=float("nan")), dict(ldh=10), dict(ldh=8)):
        a = dict(ok, **bad)
        if "ldh" not in bad:
            for sfx in ("", "_bf16io"):
                assert getattr(h, "seg_ohem_upsample_loss" + sfx)(
                    lg.data_ptr(), a["ld"], N, H, W, a["C"], yg.data_ptr(), Ho, Wo, -100, None, a["tau"], a["k"],
                    work.data_ptr(), out6.data_ptr(), S()) == 1, bad
                assert getattr(h, "seg_ohem_upsample_eval" + sfx)(
                    lg.data_ptr(), a["ld"], N, H, W, a["C"], yg.data_ptr(), Ho, Wo, -100, None, a["tau"], a["k"],
                    work.data_ptr(), out6.data_ptr(), conf.data_ptr(), S()) == 1, bad
        if "k" not in bad:
            assert h.seg_ohem_upsample_grad(
                lg.data_ptr(), a["ld"], N, H, W, a["C"], yg.data_ptr(), Ho, Wo, -100, None, a["tau"],
                work.data_ptr(), gout.data_ptr(), out6.data_ptr(), dhigh.data_ptr(), a["ldh"], S()) == 1, bad
            if "ldh" not in bad:  # the twin writes fp32 NCHW: no row stride
                assert h.seg_ohem_upsample_grad_bf16io(
                    lg.data_ptr(), a["ld"], N, H, W, a["C"], yg.data_ptr(), Ho, Wo, -100, None, a["tau"],
                    work.data_ptr(), gout.data_ptr(), out6.data_ptr(), dhigh.data_ptr(), S()) == 1, bad
    assert h.seg_ohem_upsample_eval(lg.data_ptr(), 12, N, H, W, C, yg.data_ptr(), Ho, Wo, -100, None, 0.35, 5,
                                    work.data_ptr(), out6.data_ptr(), None, S()) == 1  # confusion NULL
    torch.cuda.synchronize()
    assert torch.all(work == -3.0) and torch.all(out6 == -7.0) and torch.all(dhigh == 5.0) and int(conf.sum()) == 0
