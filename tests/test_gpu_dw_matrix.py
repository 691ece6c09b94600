"""GPU: the depthwise 3x3 kernels (csrc/dwconv.hip) per launch geometry against float64 -- the dw conv of 17 layers
of the headline model, forward (seg_dw_fwd, seg_dw_fwd_bias_act), data gradient (seg_dw_dgrad) and weight gradient
(seg_dw_wgrad + seg_conv_wgrad_reduce mode 1), with their bf16io twins.

Operands are the channel-slice views the engine hands over: every activation and gradient tensor is C columns at a
non-zero column offset (OFF_I = 8 for what a kernel reads, OFF_O = 12 for what it writes; the weight gradient reads
x at 8 and dY at 12) of a wider buffer, ld = C + 16 for the 8-offset buffer and C + 24 for the 12-offset one, so
ldin, ldout and C are pairwise different.  Buffers a kernel reads are finite outside the slice; buffers it writes are
NaN everywhere before the launch and must be NaN outside the slice and finite inside after it (with accumulate = 1
the slice holds random old values); `part` is NaN before each launch and free of NaN after.  N >= 2 wherever the
case is about geometry, so image borders fall inside the strips' row ranges.

CASES["conv"] -- (N, C, H, W), each run at stride 1 and 2, what each is for:
  (2, 36, 41, 53)  the multi-block case of both strides: forward 41 blocks at stride 1 (10332 items), 11 at stride 2
                   (2646 items), data gradient 41 blocks at both; C % 8 == 4; H and W odd; Wo % 4 == 1 (s1), 3 (s2);
                   the stride-2 data gradient's W % 4 == 1.  bias_act and the bf16io twins run here.
  (2, 960, 5, 6)   C = 960, 19 blocks at stride 1; H odd, W even; Wo % 4 == 2 (s1), Wo = 3 < 4 (s2).  bias_act and
                   the bf16io twins run here.
  (2, 8, 6, 10)    C = 8; H and W even (at stride 2 the right tap of the last column is inside the image);
                   Wo % 4 == 2 (s1), 1 (s2); the stride-2 data gradient's W % 4 == 2.
  (3, 12, 4, 7)    C % 8 == 4; H even, W odd; Wo % 4 == 3 (s1), 0 (s2); the stride-2 data gradient's W % 4 == 3.
  (2, 16, 5, 11)   Wo % 4 == 3 (s1), Wo = 6, % 4 == 2 (s2).
  (2, 20, 1, 3)    H = 1 (every row tap but the centre is padding); Wo = 3 (s1), 2 (s2).
  (2, 24, 3, 1)    W = 1: Wo = 1 at both strides, every column tap but the centre is padding.
  (2, 16, 2, 2)    W = 2: Wo = 2 (s1), 1 (s2); the stride-2 data gradient's W = 2.
  (1, 8, 1, 1)     a single pixel.
CONV_CLASSES names the launch classes and the (case, stride) pairs that claim each; tests/test_dw_geometry.py (CPU)
proves every claim from the item counts (one item per strip of seg_dw_wgrad_geometry's out[6] pixels and float4
channel group, 256 per block).  Per (case, stride) the forward runs with lazy input off and with in_act 0, 1 and 2
(shifts positive in most channels, so act(shift) != 0: padding must be exactly 0), the data gradient with
accumulate 0 and 1.

CASES["wgrad"] -- (N, C, H, W, stride) -> (row blocks, strips of the last block, RG, gy, idle lanes of the last
channel chunk, in_act of the lazy run); each runs with lazy input off and on.  The CPU file proves the numbers from
seg_dw_wgrad_geometry:
  C = 32 (RG = 32), 96 (RG = 10), 144 (RG = 7), 192 (RG = 5): at least 3 row blocks, the last one ragged;
  (5, 96, 27, 41, 1), (2, 192, 29, 29, 1), (5, 960, 21, 33, 2), (5, 384, 31, 9, 1), (5, 576, 93, 2, 1): a last block
  with fewer strips than RG (9 of 10, 2 of 5, 3 of 4, 3 of 5, 3 of 5), grids of 37, 23, 68, 46 and 69 blocks -- each
  at least 9 and no multiple of 8, so xcd_swizzle's remainder path feeds the row-block / channel-chunk split;
  C = 260: gy = 2, TC = 33, one idle lane in the last chunk (the `cg < CG` guard);
  C = 384 (gy = 2), 576 (gy = 3), 960 (gy = 4) with at least 2 row blocks -- production's classes;
  (2, 32, 2, 5, 1): one block with 8 strips for 32 row groups.

Checks.  Forward, data gradient and bias_act are compared element by element with float64 conv2d / conv2d_input
(groups = C) of the same operands, the lazy transform done in float64.  The bound is that of the operation in fp32,
u = 2^-24: 2 u (9 sum|w||x| + 2 sum|w|(|u sc| + |sh|) [lazy, in-image taps] + |bias| [bias_act] + |old|
[accumulate = 1]) -- a 9-term dot product is off by at most about 9 u sum|w||x|, the lazy affine by at most
u (|u sc| + |sh|) per tap whether fused or not, the epilogue's or the accumulate's one addition by at most
u (sum|w||x| + |bias| or |old|); the factor 2 is the headroom.  Where the bound is 0 the result must be exactly 0.
The weight gradient: every row block's slab against the float64 sum over exactly the strips the header of
csrc/dwconv.hip promises, bound 2 d u sum|dy||x| with d = tww ceil(spb / RG) + ceil(log2 RG) + 1 the longest
addition chain of the geometry; after seg_conv_wgrad_reduce (mode 1, onto a NaN dw) against float64 conv2d_weight
with d + blocks; sum|dy||x| = 0 (lazy input, fully clamped channels) requires an exact 0; the same call twice gives
the same bits.  bf16io twins on the multi-block cases with bf16-representable operands: outputs bitwise the fp32
kernel's rounded to bf16, slabs bitwise equal (the rule of tests/test_gpu_bf16io.py).  The largest error / bound
ratio per case goes to the parity record (profiles/dw_matrix_parity.jsonl).
"""
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

from seg_amd._lib import call, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
U = 2.0 ** -24
BF = torch.bfloat16
OFF_I, OFF_O = 8, 12    # column of the slice a kernel reads / writes (the weight gradient: x / dY)
PAD_I, PAD_O = 16, 24   # ld - C of those buffers

CASES = {
    "conv": {
        (2, 36, 41, 53): "multi-block at both strides, C % 8 == 4, odd H and W",
        (2, 960, 5, 6): "C = 960, 19 blocks at stride 1, Wo = 3 at stride 2",
        (2, 8, 6, 10): "C = 8, even H and W",
        (3, 12, 4, 7): "even H, odd W, Wo % 4 == 3 / 0",
        (2, 16, 5, 11): "Wo % 4 == 3 / 2",
        (2, 20, 1, 3): "H = 1",
        (2, 24, 3, 1): "W = 1",
        (2, 16, 2, 2): "W = 2",
        (1, 8, 1, 1): "one pixel",
    },
    # (N, C, H, W, stride): (row blocks, strips of the last block, RG, gy, idle lanes, lazy in_act)
    "wgrad": {
        (5, 32, 20, 13, 1): (3, 132, 32, 1, 0, 2),
        (5, 96, 13, 5, 1): (3, 42, 10, 1, 0, 2),
        (5, 96, 25, 10, 2): (3, 42, 10, 1, 0, 1),
        (5, 96, 27, 41, 1): (37, 9, 10, 1, 0, 0),
        (2, 144, 22, 5, 1): (3, 28, 7, 1, 0, 2),
        (5, 144, 19, 10, 2): (3, 32, 7, 1, 0, 2),
        (2, 192, 29, 29, 1): (23, 2, 5, 1, 0, 2),
        (2, 260, 22, 5, 1): (3, 28, 7, 2, 1, 2),
        (5, 260, 19, 10, 2): (3, 32, 7, 2, 1, 1),
        (5, 384, 31, 9, 1): (23, 3, 5, 2, 0, 2),
        (2, 576, 16, 5, 1): (3, 20, 5, 3, 0, 2),
        (5, 576, 93, 2, 1): (23, 3, 5, 3, 0, 2),
        (5, 960, 5, 5, 1): (3, 16, 4, 4, 0, 2),
        (5, 960, 21, 33, 2): (17, 3, 4, 4, 0, 2),
        (2, 32, 2, 5, 1): (1, 8, 32, 1, 0, 2),
    },
}
BIAS_ACT_CASES = ((2, 36, 41, 53), (2, 960, 5, 6))
TWIN_CASES = BIAS_ACT_CASES  # the multi-block conv cases; every weight-gradient case with several row blocks

_C0, _C960, _C8, _C12, _C16, _H1, _W1, _W2 = ((2, 36, 41, 53), (2, 960, 5, 6), (2, 8, 6, 10), (3, 12, 4, 7),
                                              (2, 16, 5, 11), (2, 20, 1, 3), (2, 24, 3, 1), (2, 16, 2, 2))
CONV_CLASSES = {
    "fwd grid >= 9, not a multiple of 8, partial last block": [(_C0, 1), (_C0, 2), (_C960, 1)],
    "dgrad grid >= 9, not a multiple of 8, partial last block": [(_C0, 1), (_C0, 2), (_C960, 1), (_C960, 2)],
    "Wo % 4 == 1": [(_C0, 1), (_C8, 2)],
    "Wo % 4 == 2": [(_C8, 1), (_C960, 1), (_C16, 2)],
    "Wo % 4 == 3": [(_C12, 1), (_C16, 1), (_C0, 2)],
    "Wo < 4": [(_H1, 1), (_W2, 1), (_C960, 2), (_H1, 2)],
    "Wo == 1": [(_W1, 1), (_W1, 2), (_W2, 2)],
    "H == 1": [(_H1, 1), (_H1, 2)],
    "H odd, W odd": [(_C0, 2)],
    "H odd, W even": [(_C960, 2)],
    "H even, W odd": [(_C12, 2)],
    "H even, W even": [(_C8, 2)],
    "dgrad W % 4 != 0": [(_C0, 2), (_C8, 2), (_C12, 2)],
    "dgrad W == 1": [(_W1, 2)],
    "dgrad W == 2": [(_W2, 2)],
    "C == 8": [(_C8, 1), (_C8, 2)],
    "C % 8 == 4": [(_C0, 1), (_C0, 2), (_C12, 1), (_C12, 2)],
    "C == 960": [(_C960, 1), (_C960, 2)],
}


def wgrad_class(blocks, last, RG, gy, idle):
    """(gy, RG a power of two, idle lanes in the last chunk, several row blocks, last block shorter than RG)."""
    return (gy, RG & (RG - 1) == 0, idle > 0, blocks > 1, last < RG)


def covered():
    """The weight-gradient launch classes this file compares with float64."""
    return {wgrad_class(*v[:5]) for v in CASES["wgrad"].values()}


# ---- geometry, operands, float64 references and bounds (no GPU: tests/test_dw_geometry.py uses them too) ---------

def cdiv(a, b):
    return -(-a // b)


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def geometry(N, Ho, Wo, C):
    out = (ctypes.c_int * 7)()
    assert query("seg_dw_wgrad_geometry", N, Ho, Wo, C, ctypes.addressof(out)) == 0
    g = dict(zip(("TC", "gy", "RG", "spb", "blocks", "tww", "tw"), out))
    g["nstrips"] = N * Ho * cdiv(Wo, g["tww"])
    g["last"] = g["nstrips"] - (g["blocks"] - 1) * g["spb"]
    g["idle"] = g["TC"] * g["gy"] - C // 4
    return g


def conv_items(N, Ho, Wo, C, tw):
    """Work items of the forward / data gradient over an N x Ho x Wo x C output."""
    return N * Ho * cdiv(Wo, tw) * (C // 4)


def chain(g):
    """The longest addition chain of a slab element: a thread's strips, the row-group tree, the product."""
    return g["tww"] * cdiv(g["spb"], g["RG"]) + (g["RG"] - 1).bit_length() + 1


def gen(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def lazy_params(C, seed):
    """scale, shift of the lazy input transform: shift positive (act(shift) != 0) except in channels c % 8 == 3;
    channels c % 16 == 6 are clamped to 0 everywhere by ReLU / ReLU6 (tiny scale, shift -50)."""
    sc, sh = gen(C, seed=seed) * 1.5, gen(C, seed=seed + 1).abs() * 1.5 + 0.5
    c = torch.arange(C)
    sh[c % 8 == 3] *= -1
    sc[c % 16 == 6] *= 1e-3
    sh[c % 16 == 6] = -50.0
    return sc, sh


def act_fn(z, act):
    return z if act == 0 else (z.clamp(min=0) if act == 1 else z.clamp(0, 6))


def lazy_apply(u, sc, sh, act):
    """(act(u sc + sh), |u sc| + |sh|) in u's dtype, NCHW.  The affine is evaluated in float64 and rounded once, which
    in fp32 is the kernels' fmaf (seg_bn_act4): the activated input is then off by one relative rounding, which is
    what lets the weight gradient's bound be a multiple of sum|dy||x| alone."""
    sc, sh = sc.double().view(1, -1, 1, 1), sh.double().view(1, -1, 1, 1)
    z = u.double() * sc
    return act_fn((z + sh).to(u.dtype), act), (z.abs() + sh.abs()).to(u.dtype)


def dw_conv(a, w, s):
    return F.conv2d(a, w.to(a.dtype), stride=s, padding=1, groups=a.shape[1])


def dw_conv_input(dy, w, s, H, W):
    N, C = dy.shape[:2]
    return torch.nn.grad.conv2d_input((N, C, H, W), w.to(dy.dtype), dy, stride=s, padding=1, groups=C)


def conv_operands(case, s):
    """fp32 operands of one (case, stride), NCHW: u, w, dy, old, bias, (sc, sh)."""
    N, C, H, W = case
    Ho, Wo = out_hw(H, W, s)
    k = 7919 * (C + 31 * H + 57 * W) + s
    return dict(u=gen(N, C, H, W, seed=k), w=gen(C, 1, 3, 3, seed=k + 1), dy=gen(N, C, Ho, Wo, seed=k + 2),
                old=gen(N, C, H, W, seed=k + 3) * 2, bias=gen(C, seed=k + 4), lazy=lazy_params(C, k + 5))


def fwd_ref(op, s, act=None, bias_act=None, dtype=torch.float64):
    """(y, bound) of the forward, NCHW.  act: the lazy input's in_act (None: off); bias_act: the epilogue's act."""
    u, w = op["u"].to(dtype), op["w"].to(dtype)
    if act is None:
        a, t = u, None
    else:
        a, t = lazy_apply(u, *op["lazy"], act)
    y = dw_conv(a, w, s)
    bound = 9 * dw_conv(a.abs(), w.abs(), s)
    if t is not None:
        bound = bound + 2 * dw_conv(t, w.abs(), s)
    if bias_act is not None:
        b = op["bias"].to(dtype).view(1, -1, 1, 1)
        y = act_fn(y + b, bias_act)
        bound = bound + b.abs()
    return y, 2 * U * bound.double()


def dgrad_ref(op, s, accumulate, dtype=torch.float64):
    u, w, dy = op["u"], op["w"].to(dtype), op["dy"].to(dtype)
    H, W = u.shape[2:]
    dx = dw_conv_input(dy, w, s, H, W)
    bound = 9 * dw_conv_input(dy.abs(), w.abs(), s, H, W)
    if accumulate:
        dx = dx + op["old"].to(dtype)
        bound = bound + op["old"].to(dtype).abs()
    return dx, 2 * U * bound.double()


def wgrad_operands(case, act):
    """fp32 x (the raw input), dy and the activated input a (float64) of one weight-gradient case, NCHW."""
    N, C, H, W, s = case
    Ho, Wo = out_hw(H, W, s)
    k = 104729 + 7919 * (C + 31 * H + 57 * W) + s
    op = dict(u=gen(N, C, H, W, seed=k), dy=gen(N, C, Ho, Wo, seed=k + 2), lazy=lazy_params(C, k + 5))
    return op


def wgrad_strips(a, dy, s, tww):
    """Per-strip sums of dy * x(tap) and of their magnitudes, [nstrips][9][C] in a's dtype: strips are tww
    consecutive output pixels of one output row in (n, ho, strip) order, the last strip of a row ragged."""
    N, C, Ho, Wo = dy.shape
    spr = cdiv(Wo, tww)
    ap = F.pad(a, (1, 1, 1, 1))
    st = torch.zeros(N * Ho * spr, 9, C, dtype=a.dtype)
    sa = torch.zeros_like(st)
    for ky in range(3):
        for kx in range(3):
            xs = ap[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]
            p = F.pad((dy * xs).permute(0, 2, 3, 1), (0, 0, 0, spr * tww - Wo))  # [N][Ho][spr * tww][C]
            st[:, 3 * ky + kx] = p.reshape(N * Ho * spr, tww, C).sum(1)
            sa[:, 3 * ky + kx] = p.abs().reshape(N * Ho * spr, tww, C).sum(1)
    return st, sa


def slabs_of(strips, g):
    """[blocks][9][C]: row block b sums the strips [b spb, min(nstrips, (b + 1) spb))."""
    return torch.stack([strips[b * g["spb"]:min(g["nstrips"], (b + 1) * g["spb"])].sum(0)
                        for b in range(g["blocks"])])


def wgrad_ref(case, act, dtype=torch.float64):
    """Slabs [blocks][9][C], their bound, dW [C][9] and its bound, the geometry; act None: lazy off."""
    N, C, H, W, s = case
    op = wgrad_operands(case, act)
    g = geometry(N, *out_hw(H, W, s), C)
    u, dy = op["u"].to(dtype), op["dy"].to(dtype)
    a = u if act is None else lazy_apply(u, *op["lazy"], act)[0]
    st, sa = wgrad_strips(a, dy, s, g["tww"])
    slabs, mags = slabs_of(st, g), slabs_of(sa, g).double()
    d = chain(g)
    dw = st.sum(0).t().contiguous()
    if dtype == torch.float64:
        want = torch.nn.grad.conv2d_weight(a, (C, 1, 3, 3), dy, stride=s, padding=1, groups=C).reshape(C, 9)
        assert float((dw - want).norm()) <= 1e-12 * float(want.norm()), "the strips sum to the weight gradient"
        dw = want
    return dict(op=op, g=g, slabs=slabs, slab_bound=2 * d * U * mags, dw=dw,
                dw_bound=2 * (d + g["blocks"]) * U * sa.sum(0).t().double())


def ratio(got, want, bound):
    """The largest |got - want| / bound; where the bound is 0 the result must be exactly 0 (else inf)."""
    err = (got.double() - want.double()).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()) or not bool(torch.isfinite(err).all()):
        return float("inf")
    r = err[~zero] / bound[~zero]
    return float(r.max()) if r.numel() else 0.0


def rows_of(t):
    """NCHW -> NHWC rows [N * H * W][C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def nchw_of(rows, N, H, W):
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2)


# ---- the launches ----------------------------------------------------------------------------------------------

def S():
    return torch.cuda.current_stream().cuda_stream


def in_buf(t, off, pad, seed, dtype=torch.float32):
    """NCHW t as the C-column slice at column `off` of a finite (C + pad)-column buffer; (buffer, slice pointer)."""
    r = rows_of(t)
    buf = gen(r.shape[0], r.shape[1] + pad, seed=seed)
    buf[:, off:off + r.shape[1]] = r
    buf = buf.to(dtype).to(DEV)
    return buf, buf.data_ptr() + off * buf.element_size(), buf.shape[1]


def out_buf(M, C, off, pad, dtype=torch.float32, old=None):
    buf = torch.full((M, C + pad), NAN)
    if old is not None:
        buf[:, off:off + C] = rows_of(old)
    buf = buf.to(dtype).to(DEV)
    return buf, buf.data_ptr() + off * buf.element_size(), buf.shape[1]


def read_out(buf, off, C, what):
    torch.cuda.synchronize()
    o = buf.cpu()
    assert bool(torch.isnan(o[:, :off]).all()) and bool(torch.isnan(o[:, off + C:]).all()), \
        (what, "a store outside the output slice")
    o = o[:, off:off + C].contiguous()
    assert bool(torch.isfinite(o).all()), (what, "an output element was never written")
    return o


def ptr(t):
    return t.data_ptr() if t is not None else None


class Worst:
    def __init__(self, case):
        self.case, self.m, self.t0 = case, {}, time.perf_counter()

    def check(self, entry, what, r):
        self.m[entry] = max(self.m.get(entry, 0.0), r)
        print(f"{entry} {self.case} {what}: error / bound {r:.3f}")
        assert r <= 1.0, (entry, self.case, what, r)

    def write(self, record):
        record(case=str(self.case), worst_ratio=self.m, test_seconds=time.perf_counter() - self.t0)


def same_bf16(b16, f32, what):
    ref = f32.to(BF)
    assert torch.equal(b16.view(torch.int16), ref.view(torch.int16)), \
        (what, f"max diff {(b16.float() - ref.float()).abs().max().item()}")


def launch_fwd(op, case, s, act, dtype=torch.float32, bias_act=None):
    """One forward launch; the output slice as rows [N * Ho * Wo][C] (on the CPU)."""
    N, C, H, W = case
    Ho, Wo = out_hw(H, W, s)
    xb, xp, ldin = in_buf(op["u"], OFF_I, PAD_I, 11, dtype)
    ob, opn, ldout = out_buf(N * Ho * Wo, C, OFF_O, PAD_O, dtype)
    wk = op["w"].view(C, 9).t().contiguous().to(DEV)
    sc, sh = (t.to(DEV) for t in op["lazy"]) if act is not None else (None, None)
    if bias_act is not None:
        b = op["bias"].to(DEV)
        call("seg_dw_fwd_bias_act", xp, ldin, N, H, W, C, wk.data_ptr(), b.data_ptr(), bias_act, opn, ldout, Ho, Wo, s,
             S())
    else:
        name = "seg_dw_fwd" if dtype == torch.float32 else "seg_dw_fwd_bf16io"
        call(name, xp, ldin, N, H, W, C, ptr(sc), ptr(sh), act if act is not None else 0, wk.data_ptr(), opn, ldout,
             Ho, Wo, s, S())
    return read_out(ob, OFF_O, C, ("fwd", case, s, act, bias_act))


def launch_dgrad(op, case, s, accumulate, dtype=torch.float32):
    N, C, H, W = case
    Ho, Wo = out_hw(H, W, s)
    gb, gp, lddy = in_buf(op["dy"], OFF_I, PAD_I, 12, dtype)
    ob, opn, lddx = out_buf(N * H * W, C, OFF_O, PAD_O, dtype, op["old"] if accumulate else None)
    wk = op["w"].view(C, 9).t().contiguous().to(DEV)
    name = "seg_dw_dgrad" if dtype == torch.float32 else "seg_dw_dgrad_bf16io"
    call(name, gp, lddy, N, Ho, Wo, C, wk.data_ptr(), opn, lddx, H, W, s, accumulate, S())
    return read_out(ob, OFF_O, C, ("dgrad", case, s, accumulate))


def launch_wgrad(op, case, act, g, dtype=torch.float32):
    """The slabs [blocks][9][C] of one launch (on the device)."""
    N, C, H, W, s = case
    Ho, Wo = out_hw(H, W, s)
    gb, gp, lddy = in_buf(op["dy"], OFF_O, PAD_O, 13, dtype)
    xb, xp, ldx = in_buf(op["u"], OFF_I, PAD_I, 14, dtype)
    sc, sh = (t.to(DEV) for t in op["lazy"]) if act is not None else (None, None)
    part = torch.full((g["blocks"], 9, C), NAN, device=DEV)
    name = "seg_dw_wgrad" if dtype == torch.float32 else "seg_dw_wgrad_bf16io"
    call(name, gp, lddy, xp, ldx, N, H, W, C, ptr(sc), ptr(sh), act if act is not None else 0, Ho, Wo, s,
         part.data_ptr(), S())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(part).any()), (case, act, "a slab element was never written")
    return part


def bf16_operands(op):
    return {k: (v.to(BF).float() if k in ("u", "dy", "old") else v) for k, v in op.items()}


# ---- the tests ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("case", sorted(CASES["conv"]), ids=lambda v: "x".join(map(str, v)))
def test_fwd_dgrad(case, stride, record):
    N, C, H, W = case
    Ho, Wo = out_hw(H, W, stride)
    worst = Worst(case + (stride,))
    op = conv_operands(case, stride)
    for act in (None, 0, 1, 2):
        want, bound = fwd_ref(op, stride, act)
        got = launch_fwd(op, case, stride, act)
        worst.check("seg_dw_fwd", f"lazy {act}", ratio(got, rows_of(want), rows_of(bound)))
    for acc in (0, 1):
        want, bound = dgrad_ref(op, stride, acc)
        got = launch_dgrad(op, case, stride, acc)
        worst.check("seg_dw_dgrad", f"accumulate {acc}", ratio(got, rows_of(want), rows_of(bound)))
    if case in BIAS_ACT_CASES:
        for act in (0, 1, 2):
            want, bound = fwd_ref(op, stride, None, bias_act=act)
            got = launch_fwd(op, case, stride, None, bias_act=act)
            worst.check("seg_dw_fwd_bias_act", f"act {act}", ratio(got, rows_of(want), rows_of(bound)))
    if case in TWIN_CASES:
        ob = bf16_operands(op)
        for act in (None, 2):
            same_bf16(launch_fwd(ob, case, stride, act, BF), launch_fwd(ob, case, stride, act), ("fwd", act))
        for acc in (0, 1):
            same_bf16(launch_dgrad(ob, case, stride, acc, BF), launch_dgrad(ob, case, stride, acc), ("dgrad", acc))
    worst.write(record)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("case", sorted(CASES["wgrad"]), ids=lambda v: "x".join(map(str, v)))
def test_wgrad_slabs(case, lazy, record):
    N, C, H, W, s = case
    act = CASES["wgrad"][case][5] if lazy else None
    worst = Worst(case + (act,))
    ref = wgrad_ref(case, act)
    g, op = ref["g"], ref["op"]
    assert g["blocks"] == query("seg_dw_wgrad_blocks", N, *out_hw(H, W, s), C) == CASES["wgrad"][case][0]
    part = launch_wgrad(op, case, act, g)
    p = part.cpu()
    for b in range(g["blocks"]):
        r = ratio(p[b], ref["slabs"][b], ref["slab_bound"][b])
        assert r <= 1.0, (case, act, f"row block {b} of {g['blocks']}", r)
    worst.check("seg_dw_wgrad", f"worst of {g['blocks']} row blocks", ratio(p, ref["slabs"], ref["slab_bound"]))
    assert torch.equal(part, launch_wgrad(op, case, act, g)), (case, act, "not reproducible")
    dw = torch.full((C, 9), NAN, device=DEV)
    call("seg_conv_wgrad_reduce", part.data_ptr(), g["blocks"], dw.data_ptr(), C, 1, 3, 1, 0, S())
    torch.cuda.synchronize()
    worst.check("seg_conv_wgrad_reduce", "dW", ratio(dw.cpu(), ref["dw"], ref["dw_bound"]))
    if g["blocks"] > 1:
        ob = bf16_operands(op)
        assert torch.equal(launch_wgrad(ob, case, act, g, BF), launch_wgrad(ob, case, act, g)), \
            (case, act, "the bf16io slabs differ from the fp32 kernel's")
    worst.write(record)
