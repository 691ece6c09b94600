"""GPU: the implicit-GEMM weight gradient (csrc/wgrad.hip, wgrad_kernel<BM, BN, WM, WN, KS, BF, IT, VW, XF>) per
tile, loader and split against float64 -- the kernel behind the weight path of convolution_backward for every 1x1
conv and both stems (src/unet.py:113,116, torchvision's InvertedResidual expand / project convs reached through
src/unet.py:15-19) and, in the bf16 programs, the dense 3x3 convs (src/unet.py:58,61).

The other kernel tests launch it at M <= 384 pixels, where seg_conv_wgrad_splits gives one split, and compare only
the sum over slabs.  Here the split count is forced (any splits >= 1 is legal, include/segamd.h) and every slab is
compared on its own with the float64 partial sum over exactly the pixel range the header promises,
[s * kchunk, min(M, (s + 1) * kchunk)), kchunk from seg_conv_wgrad_geometry -- so the same wrong range in both
operand loads, or a pixel counted in two slabs, cannot cancel.

Images: N = 2, H = 9, W = 13.  Stride 1: hw = 117, M = 234; W < 16, so every K step of the 3x3 pixel cursor wraps a
row, steps cross the image boundary, forced splits start mid-row and mid-image, and M is no multiple of 16 or 32.
Stride 2: 5 x 7 outputs, M = 70.  Split counts 1, 3, 7, 40: at M = 234 the fp32 kernel's kchunk is 240, 80, 48, 16
(7 splits: 5 filled + 2 empty; 40: 15 filled + 25 empty), the bf16-math kernels' 256, 96, 64, 32 (40: 8 filled).
An empty split must write an all-zero slab; `part` is NaN before each launch and no NaN may remain.

Operands are bf16-representable fp32 values, so the three maths (fp32; bf16 math on fp32 storage; bf16 storage) see
the same numbers, every product is exact in fp32 and one float64 reference serves all three at the project's
fp32-accumulation bound, rel-L2 1e-5 (TOL32 of tests/test_gpu_igemm_tiles.py).  dY's pad channels (Cout % 4 != 0)
and x's columns beyond Cin (ldx = Cin + 8, or Cin + 4 to force the 4-channel-slot loader on bf16 storage) are NaN:
a load that strays poisons its slab.  The stems pass Cin = 4 with a zero fourth channel, as the engine pads them.

Per case and launch: every slab against float64; the same call again gives the same bits; seg_conv_wgrad_bf16io
through either loader equals seg_conv_wgrad_bf16 on the fp32 copy bit for bit (the same MFMA order on the same
operands); seg_conv_wgrad_reduce of the slabs (accumulate 0 into NaN, then accumulate 1: twice the gradient)
against torch.nn.grad.conv2d_weight in float64 at 1e-5, with the stems' real Cin = 3.  The _xf entry points: slabs
bitwise those of the plain entry point on seg_bn_apply's output, and against float64 of that applied input (for
bf16 math on fp32 storage rounded to bf16, as the kernel rounds in LDS staging); every shift is positive, so
act(shift) != 0 in every channel and a transformed 3x3 padding tap cannot pass.

tests/test_wgrad_geometry.py (CPU) imports CASES / XF_CASES / covered() and pins the production programs' (tile,
math, xf) triples inside what runs here.
"""
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

from seg_amd._lib import call, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
N, H, W = 2, 9, 13
SPLITS = (1, 3, 7, 40)
TOL = 1e-5  # fp32 accumulation of exact products: tests/test_gpu_igemm_tiles.py TOL32, test_gpu_ops.py

# case -> ((BM, BN), ks, stride, Cin as passed, Cout, real Cin)
CASES = {
    "A1": ((128, 128), 3, 1, 16, 136, 16),    # Nw 144: second row tile and second column tile both partial
    "A2": ((128, 128), 1, 1, 136, 136, 136),  # 8-channel slots on bf16 storage
    "A3": ((128, 128), 1, 1, 132, 130, 132),  # lddy 132, two NaN pad channels; Cin % 8 != 0: 4-channel slots
    "B1": ((128, 32), 1, 1, 24, 144, 24),     # production (24 -> 144); the column tile narrower than BN
    "B2": ((128, 32), 3, 1, 8, 128, 8),       # Nw 72; fewer B load slots than threads
    "C1": ((64, 128), 1, 1, 192, 64, 192),    # production xf shape (192 -> 64)
    "C2s1": ((64, 128), 3, 1, 16, 72, 16),    # Nw 144
    "C2s2": ((64, 128), 3, 2, 16, 72, 16),
    "D1": ((64, 64), 1, 1, 16, 96, 16),
    "D2": ((64, 64), 3, 1, 4, 64, 3),         # UNet stem
    "E1": ((32, 128), 1, 1, 16, 10, 16),      # the head; lddy 12
    "E2": ((32, 128), 3, 2, 4, 32, 3),        # MobileNetV2 stem
    "E3": ((32, 128), 3, 1, 80, 32, 80),
}
XF_CASES = ("B1", "C1", "D1", "E1", "A2", "A1", "C2s1")  # the last two: 3x3, stride 1
# entry point -> (math, storage type, bf16 flag of the geometry query)
ENTRIES = {"seg_conv_wgrad": ("f32", F32, 0), "seg_conv_wgrad_bf16": ("bf16", F32, 1),
           "seg_conv_wgrad_bf16io": ("bf16io", BF, 1)}


def covered(kernel=False):
    """{(tile, math, xf)} this file runs against float64; kernel: {(tile, math, xf, ks, stride)}."""
    out = {(CASES[c][0], m, c in XF_CASES and xf) + (CASES[c][1:3] if kernel else ())
           for c in CASES for m, _, _ in ENTRIES.values() for xf in (False, True)}
    return out


def S():
    return torch.cuda.current_stream().cuda_stream


def r4(c):
    return (c + 3) & ~3


def rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def vals(rows, C, seed, scale=1.0, shift=0.0):
    """[rows][C] fp32 values exactly representable in bf16 (tests/test_gpu_views.py vals)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, C, generator=g) * scale + shift).to(BF).float()


class Geo:
    def __init__(self, case):
        self.case = case
        self.tile, self.ks, self.stride, self.cin, self.cout, self.creal = CASES[case]
        self.pad = 1 if self.ks == 3 else 0
        self.Ho = (H + 2 * self.pad - self.ks) // self.stride + 1
        self.Wo = (W + 2 * self.pad - self.ks) // self.stride + 1
        self.M, self.nw, self.lddy = N * self.Ho * self.Wo, self.ks * self.ks * self.cin, r4(self.cout)
        assert self.M == (234 if self.stride == 1 else 70)

    def kchunk(self, splits, bf16):
        """Pixels per split, from the library; the case lands on the tile it claims."""
        out = (ctypes.c_int * 3)()
        assert query("seg_conv_wgrad_geometry", self.M, self.cout, self.cin, self.ks, splits, bf16,
                     ctypes.addressof(out)) == 0
        assert (out[0], out[1]) == self.tile, (self.case, tuple(out))
        return out[2]

    def eight(self, ldx):
        """launch_wgrad's condition for the 8-channel-slot loader on bf16 storage."""
        return self.cout % 8 == 0 and self.cin % 8 == 0 and self.lddy % 8 == 0 and ldx % 8 == 0


def im2col64(g, rows):
    """float64 [M][ks*ks*Cin] (tap-major, the slab's column order) of NHWC rows [N*H*W][Cin]; padding taps are 0."""
    x = rows.double().view(N, H, W, g.cin).permute(0, 3, 1, 2)
    u = F.unfold(x, g.ks, padding=g.pad, stride=g.stride)  # [N][Cin * taps][Ho * Wo], channel-major
    return u.view(N, g.cin, g.ks * g.ks, g.Ho * g.Wo).permute(0, 3, 2, 1).reshape(g.M, g.nw)


_DATA = {}


def data(case):
    """x rows, dY rows, their float64 im2col / dY and the float64 weight gradient: once per case."""
    if case not in _DATA:
        g = Geo(case)
        k = sorted(CASES).index(case)
        x = vals(N * H * W, g.cin, 100 + k)
        x[:, g.creal:] = 0
        dy = vals(g.M, g.cout, 200 + k)
        x4 = x[:, :g.creal].double().view(N, H, W, g.creal).permute(0, 3, 1, 2)
        dy4 = dy.double().view(N, g.Ho, g.Wo, g.cout).permute(0, 3, 1, 2)
        dw = torch.nn.grad.conv2d_weight(x4, (g.cout, g.creal, g.ks, g.ks), dy4, stride=g.stride, padding=g.pad)
        _DATA[case] = dict(g=g, x=x, dy=dy, dy64=dy.double(), col=im2col64(g, x), dw=dw, parts={})
    return _DATA[case]


def slab_refs(dy64, col, M, kchunk, cache=None):
    """float64 partial dY[range].T @ im2col(x)[range] of every non-empty split."""
    if cache is not None and kchunk in cache:
        return cache[kchunk]
    refs = [dy64[lo:min(M, lo + kchunk)].t() @ col[lo:min(M, lo + kchunk)] for lo in range(0, M, kchunk)]
    if cache is not None:
        cache[kchunk] = refs
    return refs


class Worst:
    """The largest error / bound ratio per entry point of one test, for the parity record."""

    def __init__(self, g):
        self.g, self.m, self.t0 = g, {}, time.perf_counter()

    def check(self, name, err, bound, what):
        self.m[name] = max(self.m.get(name, 0.0), err / bound)
        print(f"{name} {self.g.case} {what}: {err:.3e} (bound {bound:g})")
        assert err < bound, (name, self.g.case, what, err)

    def write(self, record):
        sec = time.perf_counter() - self.t0
        for name, m in self.m.items():
            record(entry=name, tile="%dx%d" % self.g.tile, case=self.g.case, worst_margin=m, test_seconds=sec)


class Job:
    """The device operands of one case in one storage type: dY [M][lddy] with NaN pad channels, x [N*H*W][ldx] with
    NaN beyond Cin."""

    def __init__(self, g, dt, ldx, x, dy):
        self.g, self.dt, self.ldx = g, dt, ldx
        b = torch.full((g.M, g.lddy), NAN)
        b[:, :g.cout] = dy
        self.dy = b.to(dt).to(DEV)
        b = torch.full((N * H * W, ldx), NAN)
        b[:, :g.cin] = x
        self.x = b.to(dt).to(DEV)

    def launch(self, name, splits, x=None, xf=()):
        g = self.g
        part = torch.full((splits, g.cout, g.nw), NAN, device=DEV)
        call(name, self.dy.data_ptr(), g.lddy, (self.x if x is None else x).data_ptr(), self.ldx, N, H, W, g.cin,
             g.Ho, g.Wo, g.cout, g.ks, g.stride, g.pad, part.data_ptr(), splits, *xf, S())
        torch.cuda.synchronize()
        return part


def check_slabs(worst, name, part, refs, kchunk, what):
    """Every slab of one launch: non-empty splits against their float64 partial, empty ones all zero, no NaN left."""
    g = worst.g
    p = part.cpu()
    assert not bool(torch.isnan(p).any()), (name, g.case, what, "a slab element was never written")
    filled = -(-g.M // kchunk)
    assert filled == len(refs) and filled <= p.shape[0]
    errs = [rel(p[s].double(), refs[s]) for s in range(filled)]
    s = max(range(filled), key=errs.__getitem__)
    worst.check(name, errs[s], TOL, f"{what} kchunk {kchunk}: worst of {filled} slabs (slab {s})")
    for s in range(filled, p.shape[0]):
        assert int(torch.count_nonzero(p[s])) == 0, (name, g.case, what, f"empty split {s} is not all zero")


def check_reduce(worst, name, part, d, what):
    """seg_conv_wgrad_reduce of the slabs into a NaN-filled dW, then accumulated once more, against float64."""
    g = worst.g
    dw = torch.full((g.cout, g.creal, g.ks, g.ks), NAN, device=DEV)
    for acc in (0, 1):
        call("seg_conv_wgrad_reduce", part.data_ptr(), part.shape[0], dw.data_ptr(), g.cout, g.creal, g.ks, 0, acc,
             S())
        torch.cuda.synchronize()
        worst.check("seg_conv_wgrad_reduce", rel(dw.double().cpu(), (1 + acc) * d["dw"]), TOL,
                    f"{name} {what} accumulate {acc}")


def loaders(g, dt):
    """Row strides of x to run: Cin + 8 (NaN beyond Cin), and on bf16 storage, where that takes the 8-channel-slot
    loader, Cin + 4 as well, which forces the 4-channel one."""
    lds = [g.cin + 8]
    if dt == BF and g.eight(g.cin + 8):
        assert not g.eight(g.cin + 4)
        lds.append(g.cin + 4)
    return lds


@pytest.mark.parametrize("case", sorted(CASES))
def test_slabs_reduce_and_bits(case, record):
    d = data(case)
    g = d["g"]
    worst = Worst(g)
    bf16_bits = {}  # splits -> seg_conv_wgrad_bf16's slabs
    for name, (math, dt, bf16) in ENTRIES.items():
        for ldx in loaders(g, dt):
            job = Job(g, dt, ldx, d["x"], d["dy"])
            for splits in SPLITS:
                kchunk = g.kchunk(splits, bf16)
                what = f"ldx {ldx} splits {splits}"
                part = job.launch(name, splits)
                check_slabs(worst, name, part, slab_refs(d["dy64"], d["col"], g.M, kchunk, d["parts"]), kchunk, what)
                assert torch.equal(part, job.launch(name, splits)), (name, case, what, "not reproducible")
                if math == "bf16":
                    bf16_bits[splits] = part
                elif math == "bf16io":
                    assert torch.equal(part, bf16_bits[splits]), (case, what, "bf16 storage != bf16 math on fp32")
                check_reduce(worst, name, part, d, what)
    worst.write(record)


XF = {"seg_conv_wgrad": "seg_bn_apply", "seg_conv_wgrad_bf16": "seg_bn_apply",
      "seg_conv_wgrad_bf16io": "seg_bn_apply_bf16io"}  # the pass the _xf form replaces


@pytest.mark.parametrize("case", XF_CASES)
def test_xf_slabs(case, record):
    g = Geo(case)
    worst = Worst(g)
    k = sorted(CASES).index(case)
    raw = vals(N * H * W, g.cin, 300 + k, 1.5, 0.3)
    dy = data(case)["dy"]
    gen = torch.Generator().manual_seed(400 + k)
    scale = (torch.rand(g.cin, generator=gen) + 0.5).to(DEV)
    shift = (torch.rand(g.cin, generator=gen) + 0.5).to(DEV)  # act(shift) > 0 in every channel
    rows = N * H * W
    for name, (math, dt, bf16) in ENTRIES.items():
        name_xf = name + "_xf"
        for ldx in loaders(g, dt):
            job = Job(g, dt, ldx, raw, dy)
            for act in (1, 2):
                xa = torch.full((rows, ldx), NAN, device=DEV, dtype=dt)
                call(XF[name], job.x.data_ptr(), ldx, rows, g.cin, scale.data_ptr(), shift.data_ptr(), act, None, 0,
                     xa.data_ptr(), ldx, S())
                torch.cuda.synchronize()
                applied = xa[:, :g.cin].cpu()
                assert not bool(torch.isnan(applied.float()).any()) and bool(torch.isnan(xa[:, g.cin:].float()).all())
                af = applied.float()
                assert float(af.min()) >= 0 and int(torch.count_nonzero(af)) > rows * g.cin // 2
                col = im2col64(g, (applied.to(BF) if math == "bf16" else applied).float())
                dy64, refs = dy.double(), {}
                for splits in SPLITS:
                    kchunk = g.kchunk(splits, bf16)
                    what = f"ldx {ldx} act {act} splits {splits}"
                    part = job.launch(name_xf, splits, xf=(scale.data_ptr(), shift.data_ptr(), act))
                    check_slabs(worst, name_xf, part, slab_refs(dy64, col, g.M, kchunk, refs), kchunk, what)
                    assert torch.equal(part, job.launch(name, splits, x=xa)), (name, case, what, "xf != apply + plain")
    worst.write(record)
