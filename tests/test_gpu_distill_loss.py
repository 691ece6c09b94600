"""GPU: the knowledge-distillation loss kernels (csrc/loss.hip: seg_kd_upsample_loss / _grad, their _bf16io twins and
seg_low_logits_f32), called through the C ABI.

Values -- against seg_amd.losses.distill_loss_terms in fp64 on the CPU over F.interpolate(..., align_corners=True) of
the same student and teacher rows (the student's bf16-rounded for the twins), upstream gradient 0.7.  The tolerances
are tests/test_gpu_loss_options.py's, as the other families take them: 1e-5 relative (+1e-7) on loss, CE and KD, 1e-5
relative norm on the low-resolution gradient after seg_upsample_bwd.  Teacher and student are independent randn * 2,
which puts KD between 1 and 3, so the relative bound means something (asserted on the reference).

The twins -- the bf16io loss twin must return, bit for bit, the fp32 kernel's out6 on the widened rows; the row
gradient twin the fp32 kernel's rows rounded once to bf16; the fp32-NCHW gradient twin the fp32 kernel's elements.

Exact -- #valid and #out-of-range, two calls bitwise equal, KD == 0.0 and an all-zero gradient for a teacher that is
the student, NaN poisoning by an out-of-range label, the all-ignored batch.

The low-resolution gradient is taken behind seg_upsample_bwd(ac = 2), as the engine launches it for a DistillLoss: the
gather with the tap weights of the kernels' own upsample (lin_ac: the fraction of scale * dst from one fma).  With
ac = 1 the weights are lin_index's, which round the product first; at 384 source rows that puts up to 1.9e-5 on a tap
weight and 1.049e-5 on this gradient (measured, and reproduced in fp64 on the CPU with only those coordinates in fp32),
past the bound.

Measured on an MI355X: on the 12 x 20 and 5 x 7 students (768 option combinations) loss, CE and KD are within 3e-7 and
the low-resolution gradient within 5.3e-7; at 384 x 352 they are within 1e-7 and 3.5e-6 (the full-resolution gradient
3.4e-6).
"""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from seg_amd._lib import call, query
from seg_amd.losses import distill_loss_terms

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
G = 0.7  # the upstream gradient
TOL = 1e-5
KD = 0.8

BIG = (1, 4, 384, 352)  # 540 672 output pixels > 2048 blocks x 256: the grid-stride loops run more than once
SMALL = [(2, 3, 12, 20), (2, 10, 12, 20), (2, 32, 12, 20), (1, 10, 5, 7)]  # 1920 / 140 pixels: no multiple of 256
ODD = (7, 9)  # a teacher resolution unrelated to the student's
AC = 2  # seg_upsample_bwd as the engine launches it behind seg_kd_upsample_grad (the kernels' own tap weights)


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


def teacher_hw(shape, res):
    _, _, H, W = shape
    return {"same": (H, W), "out": (2 * H, 2 * W), "odd": ODD}[res]


# ---------------------------------------------------------------------------------------------------------- inputs
_CASES = {}


def case(shape, res, io=False, seed=1):
    """(student low-resolution logits, teacher low-resolution logits, labels) on the CPU, made once and shared.  The
    first two rows of image 0 are ignored.  io: the student's rows rounded to bf16 (what the twin reads)."""
    key = (shape, res, io, seed)
    if key not in _CASES:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(seed)
        low = torch.randn(N, C, H, W, generator=g) * 2
        y = torch.randint(0, C, (N, 2 * H, 2 * W), generator=g)
        y[0, :2] = -100
        Ht, Wt = teacher_hw(shape, res)
        tlow = torch.randn(N, C, Ht, Wt, generator=torch.Generator().manual_seed(seed + 100)) * 2
        if io:
            low = low.to(BF).float()
        _CASES[key] = (low, tlow, y)
    return _CASES[key]


_REFS = {}


def reference(low, tlow, y, w, ce, T, ign):
    """fp64 CPU: dict(loss, CE, KD, grad, zgrad, nvalid); zgrad is the full-resolution gradient.  Made once per case
    and shared."""
    key = (id(low), id(tlow), id(y), w is None, ce, T, ign)
    if key not in _REFS:
        size = tuple(y.shape[1:])
        lr = low.double().clone().requires_grad_(True)
        z = F.interpolate(lr, size=size, mode="bilinear", align_corners=True)
        z.retain_grad()
        u = F.interpolate(tlow.double(), size=size, mode="bilinear", align_corners=True)
        loss, CE, KDv = distill_loss_terms(z, u, y, ce, KD, T, None if w is None else w.double(), -100, ign)
        loss.backward(torch.tensor(G, dtype=torch.float64))
        _REFS[key] = dict(loss=float(loss.detach()), CE=0.0 if CE is None else float(CE), KD=float(KDv.detach()),
                          grad=lr.grad, zgrad=z.grad, nvalid=int((y != -100).sum()), keep=(low, tlow, y, w))
    return _REFS[key]


# -------------------------------------------------------------------------------------------------------- launches
class Dev:
    """A case on the device: student rows (fp32 or bf16), teacher rows, labels; ld / ldt beyond round4(C) on
    request, the pad channels NaN."""

    def __init__(self, shape, low, tlow, y, io=False, wide=False):
        self.shape, self.io = shape, io
        N, C, H, W = shape
        self.ld = r4(C) + (8 if wide else 0)
        self.ldt = r4(C) + (4 if wide else 0)
        self.Ht, self.Wt = tlow.shape[2:]
        self.lg = nhwc(low, self.ld, BF if io else torch.float32)
        self.tg = nhwc(tlow, self.ldt)
        self.yg = y.to(DEV)

    def loss(self, w, ce, T, ign, kd=KD, io=None, tg=None, ldt=None, hw=None):
        N, C, H, W = self.shape
        io = self.io if io is None else io
        out6 = torch.full((6,), -7.0, device=DEV)
        work = torch.full((query("seg_kd_workspace_floats", N * 4 * H * W),), 3e38, device=DEV)
        tg = self.tg if tg is None else tg
        Ht, Wt = hw or (self.Ht, self.Wt)
        call("seg_kd_upsample_loss" + ("_bf16io" if io else ""), self.lg.data_ptr(), self.ld, N, H, W, C,
             tg.data_ptr(), ldt or self.ldt, Ht, Wt, self.yg.data_ptr(), 2 * H, 2 * W, -100,
             w.data_ptr() if w is not None else None, ce, kd, T, int(ign), work.data_ptr(), out6.data_ptr(), S())
        return out6

    def grad(self, w, ce, T, ign, stats, kd=KD, form="rows", tg=None, ldt=None, hw=None, ldh=None):
        """The full-resolution gradient: fp32 / bf16 rows [N*Ho*Wo, ldh] (the columns beyond round4(C) keep their
        fill), or for form "nchw" (the bf16io twin) a flat fp32 [N*C*Ho*Wo + 8] whose last 8 keep theirs."""
        N, C, H, W = self.shape
        Ho, Wo = 2 * H, 2 * W
        gout = torch.tensor([G], device=DEV)
        tg = self.tg if tg is None else tg
        Ht, Wt = hw or (self.Ht, self.Wt)
        args = [self.lg.data_ptr(), self.ld, N, H, W, C, tg.data_ptr(), ldt or self.ldt, Ht, Wt, self.yg.data_ptr(),
                Ho, Wo, -100, w.data_ptr() if w is not None else None, ce, kd, T, int(ign), gout.data_ptr(),
                stats.data_ptr()]
        if form == "nchw":
            flat = torch.full((N * C * Ho * Wo + 8,), 5.0, device=DEV)
            call("seg_kd_upsample_grad_bf16io_nchw", *args, flat.data_ptr(), S())
            assert bool((flat[-8:] == 5.0).all())
            return flat
        ldh = ldh or r4(C) + 4
        d = torch.full((N * Ho * Wo, ldh), 5.0, device=DEV, dtype=BF if self.io else torch.float32)
        call("seg_kd_upsample_grad" + ("_bf16io" if self.io else ""), *args, d.data_ptr(), ldh, S())
        assert bool((d[:, r4(C):] == 5.0).all())
        return d

    def low_grad(self, d, form="rows"):
        """fp32 low-resolution gradient [N, C, H, W] (CPU) of an fp32 full-resolution one, through seg_upsample_bwd."""
        N, C, H, W = self.shape
        din = torch.full((N * H * W, r4(C)), 9.0, device=DEV)
        if form == "nchw":
            call("seg_upsample_bwd", d.data_ptr(), 0, 1, N, 2 * H, 2 * W, C, din.data_ptr(), r4(C), H, W, AC, 0, S())
        else:
            call("seg_upsample_bwd", d.data_ptr(), d.shape[1], 0, N, 2 * H, 2 * W, C, din.data_ptr(), r4(C), H, W, AC,
                 0, S())
        return from_nhwc(din, N, C, H, W)


def close(got, want):
    return abs(got - want) <= TOL * abs(want) + 1e-7


def check_values(dev, low, tlow, y, w, ce, T, ign, tag):
    """One option combination of one case against the fp64 oracle; returns what missed."""
    ref = reference(low, tlow, y, w, ce, T, ign)
    assert 0.3 < ref["KD"] < 4.0, ref["KD"]  # a relative bound means something
    wg = None if w is None else w.to(DEV)
    st = dev.loss(wg, ce, T, ign)
    torch.cuda.synchronize()
    s = st.tolist()
    miss = []
    for name, got, want in (("loss", s[0], ref["loss"]), ("CE", s[4], ref["CE"]), ("KD", s[5], ref["KD"])):
        if not close(got, want):
            miss.append((tag, name, got, want))
    assert s[2] == 0.0 and s[3] == ref["nvalid"], (tag, s)
    if w is None:
        assert s[1] == ref["nvalid"], (tag, s)
    if dev.io:
        # the twins against the fp32 kernels on the widened rows: bit for bit / rounded once
        f32 = Dev(dev.shape, low, tlow, y, io=False, wide=dev.ld > r4(dev.shape[1]))
        sf = f32.loss(wg, ce, T, ign)
        assert torch.equal(st.view(torch.int32), sf.view(torch.int32)), (tag, st, sf)
        C = dev.shape[1]
        rows = f32.grad(wg, ce, T, ign, sf)
        twin = dev.grad(wg, ce, T, ign, st)
        assert torch.equal(twin[:, :r4(C)], rows[:, :r4(C)].to(BF)), tag
        flat = dev.grad(wg, ce, T, ign, st, form="nchw")
        N, _, H, W = dev.shape
        planes = flat[:-8].view(N, C, 2 * H, 2 * W).permute(0, 2, 3, 1).reshape(-1, C)
        assert torch.equal(planes, rows[:, :C]), tag
        gl = dev.low_grad(flat, "nchw")
        full = flat[:-8].view(N, C, 2 * H, 2 * W)
    else:
        N, C, H, W = dev.shape
        d = dev.grad(wg, ce, T, ign, st)
        gl = dev.low_grad(d)
        full = from_nhwc(d, N, C, 2 * H, 2 * W)
    e, ef = rel(gl, ref["grad"]), rel(full, ref["zgrad"])
    print(f"{tag}: loss {s[0]:.7f} / {ref['loss']:.7f}  CE {s[4]:.7f} / {ref['CE']:.7f}  KD {s[5]:.7f} / "
          f"{ref['KD']:.7f}  low-resolution gradient {e:.2e}  full-resolution gradient {ef:.2e}")
    if not e <= TOL:
        miss.append((tag, "gradient", e))
    if not ef <= TOL:  # the gradient kernel's own output, before seg_upsample_bwd
        miss.append((tag, "full-resolution gradient", ef))
    return miss


# ----------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
@pytest.mark.parametrize("res", ["same", "out", "odd"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_values(shape, res, io):
    """Every T, both kd_ignored, weights on / off, ce 1 / 0; the rows with ld / ldt beyond round4(C) for T = 2."""
    low, tlow, y = case(shape, res, io)
    w = weights(shape[1])
    devs = {False: Dev(shape, low, tlow, y, io), True: Dev(shape, low, tlow, y, io, wide=True)}
    miss = []
    for T, ign, weighted, ce in itertools.product((1.0, 2.0, 4.0), (True, False), (False, True), (1.0, 0.0)):
        for wide in ((False, True) if T == 2.0 else (False,)):
            tag = (f"{shape} {res} {'bf16io' if io else 'f32'} T{T:g} ign{int(ign)} w{int(weighted)} ce{ce:g} "
                   f"wide{int(wide)}")
            miss += check_values(devs[wide], low, tlow, y, w if weighted else None, ce, T, ign, tag)
    assert not miss, miss


def test_values_when_the_grid_stride_loop_runs_more_than_once():
    """540 672 output pixels.  Measured on an MI355X: loss, CE and KD within 1e-7, the full-resolution gradient
    3.4e-6 and the low-resolution gradient 3.5e-6 -- both are the fp32 rounding of `scale` in the source coordinate;
    behind seg_upsample_bwd(ac = 1) the latter was at 1.049e-5 (module docstring)."""
    low, tlow, y = case(BIG, "out")
    dev = Dev(BIG, low, tlow, y)
    assert y.numel() > 2048 * 256
    miss = check_values(dev, low, tlow, y, weights(BIG[1]), 1.0, 2.0, True, "big out f32")
    assert not miss, miss


# ------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
def test_two_calls_agree_bitwise(io):
    shape = SMALL[1]
    low, tlow, y = case(shape, "odd", io)
    dev = Dev(shape, low, tlow, y, io, wide=True)
    w = weights(shape[1]).to(DEV)
    a = dev.loss(w, 1.0, 2.0, True)
    b = dev.loss(w, 1.0, 2.0, True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ga, gb = dev.grad(w, 1.0, 2.0, True, a), dev.grad(w, 1.0, 2.0, True, b)
    C = shape[1]
    assert torch.equal(ga[:, :r4(C)].view(torch.int16 if io else torch.int32),
                       gb[:, :r4(C)].view(torch.int16 if io else torch.int32))


@pytest.mark.parametrize("T", [1.0, 2.0, 4.0, 3.0])
@pytest.mark.parametrize("shape", SMALL[:2] + SMALL[3:], ids=lambda s: "x".join(map(str, s)))
def test_a_teacher_that_is_the_student_gives_exact_zeros(shape, T):
    """Teacher rows bit for bit the student's at the same resolution (another leading dimension): q and s come from
    one device function, so KD is exactly 0.0 and, with ce = 0, the gradient all zeros (fp32 kernels)."""
    low, _, y = case(shape, "same")
    dev = Dev(shape, low, low, y, wide=True)
    assert dev.ld != dev.ldt
    for ign in (True, False):
        st = dev.loss(None, 0.0, T, ign)
        assert st[5].item() == 0.0 and st[0].item() == 0.0 and st[4].item() == 0.0, st
        d = dev.grad(None, 0.0, T, ign, st)
        assert not d[:, :r4(shape[1])].any()
        st = dev.loss(None, 1.0, T, ign)  # with the hard term: KD still exactly 0, the loss is ce CE
        assert st[5].item() == 0.0 and st[0].item() == st[4].item() > 0.0, st


@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
def test_an_out_of_range_label_poisons_loss_and_gradient(io):
    shape = SMALL[1]
    low, tlow, y = case(shape, "same", io)
    y = y.clone()
    y[1, 5, 5] = shape[1]
    y[1, 6, 7] = -3
    y[0, 9, 1] = 1 << 40
    dev = Dev(shape, low, tlow, y, io)
    for ign in (True, False):
        st = dev.loss(None, 1.0, 2.0, ign)
        assert math.isnan(st[0].item()) and st[2].item() == 3.0, st
        assert st[3].item() == int((y != -100).sum()) - 3
        N, C, H, W = shape
        bad = (y != -100) & ((y < 0) | (y >= C))
        # every pixel of P carries the NaN in all its classes; the others (kd_ignored off: ignored or out of range,
        # where the loss already is NaN) are zero
        want = torch.ones_like(bad) if ign else ((y != -100) & ~bad)
        for form in (("rows", "nchw") if io else ("rows",)):
            d = dev.grad(None, 1.0, 2.0, ign, st, form=form)
            if form == "nchw":
                body = d[:-8].view(N, C, 2 * H, 2 * W).permute(0, 2, 3, 1).reshape(-1, C)
            else:
                body = d[:, :C].float()
            isnan = torch.isnan(body).cpu()
            assert torch.equal(isnan.all(1), want.reshape(-1)) and torch.equal(isnan.any(1), want.reshape(-1))
            assert not body[~want.reshape(-1).to(DEV)].any()


def test_all_labels_ignored():
    shape = SMALL[1]
    low, tlow, y = case(shape, "odd")
    y = torch.full_like(y, -100)
    dev = Dev(shape, low, tlow, y)
    ref = reference(low, tlow, y, None, 0.0, 2.0, True)
    st = dev.loss(None, 0.0, 2.0, True)  # the teacher supervises every pixel: finite
    assert close(st[0].item(), ref["loss"]) and close(st[5].item(), ref["KD"]) and st[3].item() == 0.0
    d = dev.grad(None, 0.0, 2.0, True, st)
    assert rel(dev.low_grad(d), ref["grad"]) <= TOL
    st = dev.loss(None, 1.0, 2.0, True)  # the hard term is 0/0, as nn.CrossEntropyLoss; KD stays finite
    assert math.isnan(st[0].item()) and math.isnan(st[4].item()) and close(st[5].item(), ref["KD"])
    st = dev.loss(None, 0.0, 2.0, False)  # P = V is empty
    assert math.isnan(st[0].item()) and math.isnan(st[5].item())


# ------------------------------------------------------------------------------------------------ seg_low_logits_f32
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
@pytest.mark.parametrize("C,ld,ldo", [(10, 12, 12), (10, 24, 12), (3, 8, 4), (32, 32, 32), (5, 16, 16), (1, 4, 8)])
def test_low_logits_copy(C, ld, ldo, io):
    rows = 2 * 9 * 13  # no multiple of 256 quads for most ldo
    g = torch.Generator().manual_seed(C)
    src = torch.full((rows, ld), float("nan"))
    src[:, :C] = torch.randn(rows, C, generator=g) * 3
    sg = src.to(DEV, BF if io else torch.float32)
    out = torch.full((rows + 1, ldo), 7.0, device=DEV)
    call("seg_low_logits_f32" + ("_bf16io" if io else ""), sg.data_ptr(), ld, rows, C, out.data_ptr(), ldo, S())
    assert torch.equal(out[:rows, :C], sg[:, :C].float())  # exact copy / exact widening
    assert not out[:rows, C:].any() and bool((out[rows] == 7.0).all())
