"""GPU: every tile configuration of the implicit-GEMM template (csrc/igemm_impl.h, kTiles[0..14]) against a float64
conv2d of the same operands -- the kernel behind nn.Conv2d of src/unet.py:58,61,113,116 and torchvision's 1x1
expand / project convs (src/unet.py:15-19), their data gradients and the batch-1 inference convs.

The cost model (pick_tile) returns tile 7 at almost every small shape, so the other kernel tests never launch
tiles 0-6 and 8-14.  Here the tile is forced (engine.force_tiles / the `tile` argument of the _ic entry points) and
each entry point runs one output geometry on it, through every loader / K-chunk path of launch_igemm:

  M = 300 rows (1 x 15 x 20): BM 256 -> 256 + 44, BM 128 -> 128 + 128 + 44, BM 64 -> 4 x 64 + 44;
  Cout = 266: BN 256 -> 256 + 10, 160 -> 160 + 106, 128 -> 2 x 128 + 10, 96 -> 2 x 96 + 74, 64 -> 4 x 64 + 10,
  32 -> 8 x 32 + 10; 266 = 66 * 4 + 2 = 33 * 8 + 2, so the last 16-byte output vector is partial (scalar tail store)
  on fp32 and on bf16 storage.

in / add / out are channel-slice views (ld > C, offset != 0) of wider buffers; the out and add buffers are NaN
outside the slice and the out buffer must still be NaN there after every launch.

Checks per tile: the output against float64 (16-bit math: of the operands rounded to bf16 / f16 first, so the bound
stays at fp32 accumulation: rel 1e-5; bf16 storage: 4e-3, one rounding of the stored value); bitwise the same call
with the cost model's tile ("tile choice never changes results", csrc/igemm.hip); the BN-statistics partials and the
BN-backward partials against float64 sums over each row tile (rel 1e-5) -- not against another kernel.

The BN-statistics partials are those of conv + bias from the fp32 accumulators, before the addend (the engine never
passes both): the reference rows are the kernel's own stored output of the same launch without the addend, and
the partials of the launch with the addend must equal that launch's bitwise.
"""
import contextlib
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_splitk_ic import check_epoch_words  # noqa: E402

from seg_amd import engine  # noqa: E402
from seg_amd._lib import call, query  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")

# include/segamd.h's tile table: (BM, BN)
TILES = [(128, 128), (64, 128), (128, 64), (64, 64), (128, 96), (128, 160), (256, 32), (128, 32),
         (128, 128), (128, 128), (256, 128), (128, 256), (128, 64), (256, 64), (64, 128)]
M, HO, WO, COUT = 300, 15, 20, 266
LDO, OFF_O = 288, 8    # out: a 266-column slice at column 8 of a 288-column buffer
LDA, OFF_A = 296, 16   # add: ... at column 16 of a 296-column buffer
LDY, OFF_Y = 280, 8    # the BN layer's pre-BN output (seg_conv_igemm_bnout*'s `by`)
OFF_I = 8              # in: Cin columns at column 8 of an r8(Cin) + 16 column buffer
CASES = {  # ks, stride, pad, Cin, H, W
    "a": (3, 1, 1, 80, 15, 20),   # K 720: uniform-tap loader, chunks spanning two taps; BK 32 (16-bit operands: 64)
    "b": (3, 1, 1, 64, 15, 20),   # K 576: uniform-tap, tap-aligned chunks
    "c": (1, 1, 0, 144, 15, 20),  # K 144: BK 16 (K % 32 != 0, K < 512)
    "d": (1, 1, 0, 64, 15, 20),   # K 64: BK 16
    "e": (3, 2, 1, 4, 30, 40),    # the stem: general loader, K 36 (fp32 storage only)
    "f": (3, 1, 1, 12, 15, 20),   # Cin % 8 != 0: the general loader on bf16 storage (bf16io only)
}
TOL32, TOL16 = 1e-5, 4e-3  # tests/test_gpu_ops.py, test_gpu_bf16.py (fp32 stored); test_gpu_igemm2.py (bf16 stored)
_TILE = -1
_DATA, _REF, _FREE = {}, {}, {}


@pytest.fixture(autouse=True, params=range(15), ids=lambda t: f"tile{t}")
def tile(request):
    global _TILE
    _TILE = request.param
    engine.force_tiles(igemm=_TILE)  # also drops every memoised tile-dependent plan and route
    try:
        yield _TILE
    finally:
        _TILE = -1
        engine.force_tiles(igemm=-1)


@contextlib.contextmanager
def unforced():
    engine.force_tiles(igemm=-1)
    try:
        yield
    finally:
        engine.force_tiles(igemm=_TILE)


def free(key, fn):
    """fn() under the cost model's tile: once per key, shared by the fifteen tiles."""
    if key not in _FREE:
        with unforced():
            _FREE[key] = fn()
    return _FREE[key]


def S():
    return torch.cuda.current_stream().cuda_stream


def r8(c):
    return (c + 7) & ~7


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def gen(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rd(t, mode):
    """The operand rounding of a conv math (RNE), back in float64."""
    return (t.to(BF) if mode == "bf16" else t.to(torch.float16) if mode == "f16" else t).double()


def data(case):
    if case not in _DATA:
        ks, stride, pad, cin, H, W = CASES[case]
        k = ord(case)
        _DATA[case] = dict(x=gen(1, cin, H, W, seed=10 * k + 1),
                           w=gen(COUT, cin, ks, ks, seed=10 * k + 2) * (2.0 / (cin * ks * ks)) ** 0.5,
                           b=gen(COUT, seed=10 * k + 3), add=gen(M, COUT, seed=10 * k + 4))
    return _DATA[case]


def conv64(case, mode, x=None, tag=""):
    """float64 conv + bias of the rounded operands as [M][COUT] rows: once per (case, math)."""
    key = (case, mode, tag)
    if key not in _REF:
        ks, stride, pad, cin, H, W = CASES[case]
        d = data(case)
        y = F.conv2d(rd(d["x"], mode) if x is None else x, rd(d["w"], mode), d["b"].double(), stride=stride,
                     padding=pad)
        assert tuple(y.shape) == (1, COUT, HO, WO)
        _REF[key] = y.permute(0, 2, 3, 1).reshape(M, COUT)
    return _REF[key]


def act64(v, act):
    return v.clamp(min=0) if act == 1 else v.clamp(0, 6) if act == 2 else v


def want(case, mode, dt, act=0, x=None, tag=""):
    """act(conv + bias + addend as stored)."""
    return act64(conv64(case, mode, x, tag) + data(case)["add"].to(dt).double(), act)


def pack(w, cin, ks, w16):
    ldk = r8(ks * ks * cin)
    wk = torch.zeros(COUT * ldk, device=DEV, dtype=BF if w16 else F32)
    table, n, blocks = engine.pack_table([(w.data_ptr(), wk.data_ptr(), COUT, cin, ks, ldk, 16 if w16 else 0, cin)],
                                         w.device)
    call("seg_pack_batch", table.data_ptr(), n, blocks, S())
    return wk, ldk


class Job:
    """The device operands of one case in one storage type, as the channel-slice views the engine hands over."""

    def __init__(self, case, dt, w16=False, x=None):
        self.case, self.dt, self.es = case, dt, 2 if dt == BF else 4
        self.ks, self.stride, self.pad, self.cin, self.H, self.W = CASES[case]
        d = data(case)
        rows = (d["x"] if x is None else x).permute(0, 2, 3, 1).reshape(-1, self.cin)
        self.ldin = r8(self.cin) + 16
        buf = gen(rows.shape[0], self.ldin, seed=7)  # finite neighbours
        buf[:, OFF_I:OFF_I + self.cin] = rows
        self.inb = buf.to(dt).to(DEV)
        buf = torch.full((M, LDA), NAN)
        buf[:, OFF_A:OFF_A + COUT] = d["add"]
        self.addb = buf.to(dt).to(DEV)
        self.bias = d["b"].to(DEV)
        self.w = d["w"].to(DEV)
        self.wk, self.ldk = pack(self.w, self.cin, self.ks, w16)

    def out(self):
        return torch.full((M, LDO), NAN, dtype=self.dt, device=DEV)

    def optr(self, ob):
        return ob.data_ptr() + OFF_O * self.es

    def add(self, on=True):
        return (self.addb.data_ptr() + OFF_A * self.es, LDA) if on else (None, 0)

    def head(self, ob, bias=True, addend=True):
        """The arguments every forward entry point starts with: in ... ldadd."""
        return (self.inb.data_ptr() + OFF_I * self.es, self.ldin, 1, self.H, self.W, self.cin, self.wk.data_ptr(),
                self.ldk, self.bias.data_ptr() if bias else None, self.optr(ob), LDO, HO, WO, COUT, self.ks,
                self.stride, self.pad, *self.add(addend))


def taken(ob):
    """The output slice, once the buffer's other columns are seen to be NaN still."""
    torch.cuda.synchronize()
    o = ob.float().cpu()
    assert bool(torch.isnan(o[:, :OFF_O]).all()) and bool(torch.isnan(o[:, OFF_O + COUT:]).all()), \
        "a store outside the output slice"
    return ob[:, OFF_O:OFF_O + COUT].cpu()


def untouched(ob):
    torch.cuda.synchronize()
    return bool(torch.isnan(ob.float()).all())


def row_tiles():
    rows = ctypes.c_int(0)
    n = query("seg_conv_igemm_row_tiles", M, COUT, ctypes.addressof(rows))
    return n, rows.value


class Worst:
    """The largest error / bound ratio of one test, per entry point, for the parity record."""

    def __init__(self):
        self.m = {}

    def check(self, name, err, bound, what):
        self.m[name] = max(self.m.get(name, 0.0), err / bound)
        print(f"{name} tile {_TILE} {what}: {err:.3e} (bound {bound:g})")
        assert err < bound, (name, _TILE, what, err)

    def write(self, record):
        for name, m in self.m.items():
            record(entry=name, tile=_TILE, worst_margin=m)


# ---- seg_conv_igemm: bias + addend + BN-statistics partials ------------------------------------------------------

def plain_stat(job, addend):
    ntl, tr = row_tiles()
    ob = job.out()
    stat = torch.full((ntl, 2, COUT), NAN, device=DEV)
    call("seg_conv_igemm", *job.head(ob, addend=addend), stat.data_ptr(), S())
    return taken(ob), stat.cpu(), ntl, tr


def test_conv_igemm_and_bn_partials(tile, record):
    worst = Worst()
    bm = TILES[tile][0]
    for case in "abcde":
        job = Job(case, F32)
        got, stat, ntl, tr = plain_stat(job, True)
        assert (ntl, tr) == (-(-M // bm), bm) and M - (ntl - 1) * tr == 44
        worst.check("seg_conv_igemm", rel(got, want(case, "f32", F32)), TOL32, f"case {case} vs fp64")
        assert torch.equal(got, free(("plain", case), lambda: plain_stat(job, True)[0])), (case, "tile changes result")
        # the partials: of conv + bias, the stored output of the launch without the addend
        y0, stat0, _, _ = plain_stat(job, False)
        assert torch.equal(stat, stat0), (case, "the addend entered the BN partials")
        y0 = y0.double()
        for t in range(ntl):
            blk = y0[t * tr:min((t + 1) * tr, M)]
            worst.check("seg_conv_igemm", rel(stat[t, 0], blk.sum(0)), 1e-5, f"case {case} tile-sum {t}")
            worst.check("seg_conv_igemm", rel(stat[t, 1], ((blk - blk.mean(0)) ** 2).sum(0)), 1e-5,
                        f"case {case} tile-M2 {t}")
        st = torch.full((4, COUT), NAN, device=DEV)
        rm, rv = torch.zeros(COUT, device=DEV), torch.ones(COUT, device=DEV)
        sd = stat.to(DEV)
        call("seg_bn_stats_tiles", sd.data_ptr(), ntl, tr, M, COUT, None, None, 1e-5, 0.1, rm.data_ptr(),
             rv.data_ptr(), None, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), S())
        torch.cuda.synchronize()
        var = y0.var(0, unbiased=False)
        worst.check("seg_bn_stats_tiles", rel(st[0], y0.mean(0)), 1e-5, f"case {case} mean")
        worst.check("seg_bn_stats_tiles", rel(st[1], 1 / torch.sqrt(var + 1e-5)), 1e-5, f"case {case} invstd")
        worst.check("seg_bn_stats_tiles", rel(rv, 0.9 + 0.1 * y0.var(0, unbiased=True)), 1e-5, f"case {case} rv")
    worst.write(record)


# ---- seg_conv_igemm_act / _bf16 / _f16: epilogue activation, split-K ---------------------------------------------

MATH = {"seg_conv_igemm_act": "f32", "seg_conv_igemm_bf16": "bf16", "seg_conv_igemm_f16": "f16"}


def splits_for(case):
    ks, _, _, cin, _, _ = CASES[case]
    s = query("seg_conv_igemm_splits", 4096, COUT, cin, ks)
    return s if s > 1 else 3


def act_launch(name, job, act, splits):
    ob = job.out()
    work = torch.full((splits * M * COUT,), NAN, device=DEV) if splits > 1 else None
    call(name, *job.head(ob), None, act, work.data_ptr() if splits > 1 else None, splits, S())
    return taken(ob)


@pytest.mark.parametrize("name", sorted(MATH))
def test_conv_act_math_and_splitk(tile, record, name):
    worst = Worst()
    mode = MATH[name]
    for case in "abcde":
        job = Job(case, F32)
        for splits in (1, splits_for(case)) if case == "a" else (1,):
            for act in (1, 2):
                got = act_launch(name, job, act, splits)
                worst.check(name, rel(got, want(case, mode, F32, act)), TOL32,
                            f"case {case} act {act} splits {splits} vs fp64")
                assert torch.equal(got, free((name, case, act, splits), lambda: act_launch(name, job, act, splits))), \
                    (case, act, splits, "tile changes result")
    worst.write(record)


# ---- seg_conv_igemm_bf16io / _w16: bf16 storage ------------------------------------------------------------------

def io_launch(name, job, bias=True):
    ob = job.out()
    call(name, *job.head(ob, bias=bias), None, S())
    return taken(ob)


@pytest.mark.parametrize("name", ["seg_conv_igemm_bf16io", "seg_conv_igemm_bf16io_w16"])
def test_conv_bf16io(tile, record, name):
    worst = Worst()
    w16 = name.endswith("_w16")
    for case in "abcdf":
        job = Job(case, BF, w16)
        got = io_launch(name, job)
        worst.check(name, rel(got, want(case, "bf16", BF)), TOL16, f"case {case} vs fp64")
        assert torch.equal(got, free((name, case), lambda: io_launch(name, job))), (case, "tile changes result")
        if w16:  # igemm_impl.h: "bitwise the fp32-weight kernel: the RNE rounding is the same, done once at pack time"
            assert torch.equal(got, io_launch("seg_conv_igemm_bf16io", Job(case, BF, False))), (case, "w16 != fp32 pack")
    worst.write(record)


# ---- the lazy-BN forwards: A = act(in * xs + xb) formed on load ---------------------------------------------------

XF = {"seg_conv_igemm_xf": ("f32", F32, False), "seg_conv_igemm_bf16_xf": ("bf16", F32, False),
      "seg_conv_igemm_bf16io_xf": ("bf16", BF, False), "seg_conv_igemm_bf16io_xf_w16": ("bf16", BF, True)}


def xf_data(case, exact):
    """x, xs, xb.  exact (the 16-bit operand types): x and xb multiples of 1/16, |x| <= 4, |xb| <= 2, xs a signed
    power of two in [0.5, 2], so x xs + xb is a multiple of 1/16 below 16 in magnitude -- 8 significant bits, exact in
    fp32, bf16 and f16: the operand the kernel rounds is the reference's, whatever the order of its fp32 steps, and
    the bound stays at fp32 accumulation (a one-ulp bf16 flip of one operand alone would cost about 2e-5 here)."""
    cin, H, W = CASES[case][3:]
    g = torch.Generator().manual_seed(ord(case) + 100)
    if not exact:
        return data(case)["x"], gen(cin, seed=31) * 0.5 + 1.0, gen(cin, seed=32) + 1.0
    x = torch.randint(-64, 65, (1, cin, H, W), generator=g).float() / 16
    xs = torch.tensor([0.5, 1.0, 2.0, -0.5, -1.0, -2.0])[torch.randint(0, 6, (cin,), generator=g)]
    xb = torch.randint(-32, 33, (cin,), generator=g).float() / 16
    return x, xs, xb


def xf_launch(name, job, xs, xb, in_act):
    ob = job.out()
    call(name, *job.head(ob), None, xs.data_ptr(), xb.data_ptr(), in_act, S())
    return taken(ob)


@pytest.mark.parametrize("name", sorted(XF))
def test_conv_xf(tile, record, name):
    worst = Worst()
    mode, dt, w16 = XF[name]
    for case in "ac":
        x, xs, xb = xf_data(case, mode != "f32")
        cin = CASES[case][3]
        a = act64(x.double() * xs.double().view(1, cin, 1, 1) + xb.double().view(1, cin, 1, 1), 2)
        if mode != "f32":
            assert torch.equal(rd(a, "bf16"), a) and torch.equal(rd(x, "bf16"), x.double())
        # conv2d pads the transformed tensor: an out-of-image tap contributes 0, not act(xb)
        ref = want(case, mode, dt, 0, x=a, tag="xf")
        job = Job(case, dt, w16, x=x)
        xsd, xbd = xs.to(DEV), xb.to(DEV)
        got = xf_launch(name, job, xsd, xbd, 2)
        worst.check(name, rel(got, ref), TOL16 if dt == BF else TOL32, f"case {case} vs fp64")
        assert torch.equal(got, free((name, case), lambda: xf_launch(name, job, xsd, xbd, 2))), \
            (case, "tile changes result")
    worst.write(record)


# ---- seg_conv_igemm_bnout*: the data gradient that also reduces the BN backward -----------------------------------

BNOUT = {"seg_conv_igemm_bnout": (F32, False, "seg_conv_igemm"),
         "seg_conv_igemm_bnout_bf16io": (BF, False, "seg_conv_igemm_bf16io"),
         "seg_conv_igemm_bnout_bf16io_w16": (BF, True, "seg_conv_igemm_bf16io_w16")}
_BN = {}


def bn_layer(dt):
    """The BN layer whose dA the conv completes: its pre-BN output y (as stored), batch statistics and affine, with
    no element's y scale + shift within 1e-4 of 0 or 6 (offenders moved by multiples of 1e-2, as
    test_batchnorm_train keeps its elements off the thresholds), so the float64 mask is the only possible mask."""
    if dt not in _BN:
        g = torch.Generator().manual_seed(77)
        y = (torch.randn(M, COUT, generator=g) * 2).to(dt)
        gamma = torch.rand(COUT, generator=g) + 0.5
        beta = torch.randn(COUT, generator=g) * 0.2
        for it in range(1, 20):
            y64 = y.double()
            mean = y64.mean(0).float()
            invstd = (1 / torch.sqrt(y64.var(0, unbiased=False) + 1e-5)).float()
            scale = gamma * invstd
            shift = beta - mean * scale
            z = y64 * scale.double() + shift.double()
            bad = (z.abs() < 1e-4) | ((z - 6).abs() < 1e-4)
            if not bool(bad.any()):
                break
            y = torch.where(bad, (y.float() + 1e-2 * it).to(dt), y)
        assert not bool(bad.any()), "an element on an activation threshold"
        _BN[dt] = dict(y=y, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=shift, z=z)
    return _BN[dt]


def mask64(z, act):
    return (z > 0).double() if act == 1 else ((z > 0) & (z < 6)).double() if act == 2 else torch.ones_like(z)


@pytest.mark.parametrize("name", sorted(BNOUT))
def test_conv_bnout(tile, record, name):
    worst = Worst()
    dt, w16, plain = BNOUT[name]
    ok = 64 % (TILES[tile][1] // (8 if dt == BF else 4)) == 0  # one column vector per lane in the staged store
    assert query("seg_conv_igemm_bnout_ok", M, COUT, int(dt == BF)) == int(ok)
    assert ok == (tile not in (4, 5))
    bn = bn_layer(dt)
    yb = torch.full((M, LDY), NAN)
    yb[:, OFF_Y:OFF_Y + COUT] = bn["y"].float()
    yb = yb.to(dt).to(DEV)
    dev = {k: bn[k].to(DEV) for k in ("gamma", "mean", "invstd", "scale", "shift")}
    ntl, tr = row_tiles()
    y64 = bn["y"].double()
    for case in "bc":
        job = Job(case, dt, w16)
        ref_out = io_launch(plain, job, bias=False)
        for bact in (0, 1, 2):
            ob = job.out()
            part = torch.full((ntl, 2, COUT), NAN, device=DEV)
            rc = query(name, job.inb.data_ptr() + OFF_I * job.es, job.ldin, 1, job.H, job.W, job.cin,
                       job.wk.data_ptr(), job.ldk, job.optr(ob), LDO, COUT, job.ks, *job.add(), yb.data_ptr() +
                       OFF_Y * job.es, LDY, dev["scale"].data_ptr(), dev["shift"].data_ptr(), dev["mean"].data_ptr(),
                       bact, part.data_ptr(), S())
            if not ok:  # refused: an error code, nothing launched
                assert rc != 0 and untouched(ob) and untouched(part), (case, bact)
                continue
            assert rc == 0
            got = taken(ob)
            assert torch.equal(got, ref_out), (case, bact, "the output is the plain launch's")
            # dz on the values as stored, mask in float64 (no element near a threshold)
            dz = got.double() * mask64(bn["z"], bact)
            part = part.cpu()
            for t in range(ntl):
                r = slice(t * tr, min((t + 1) * tr, M))
                worst.check(name, rel(part[t, 0], dz[r].sum(0)), 1e-5, f"case {case} bact {bact} sum dz {t}")
                worst.check(name, rel(part[t, 1], (dz[r] * (y64[r] - bn["mean"].double())).sum(0)), 1e-5,
                            f"case {case} bact {bact} sum dz (y - mean) {t}")
            # finalized: dgamma / dbeta of F.batch_norm + activation in float64, fed the stored dA
            coef, dg, db = (torch.full((n,), NAN, device=DEV) for n in (3 * COUT, COUT, COUT))
            pd = part.to(DEV)
            call("seg_bn_bwd_finalize_tiles", pd.data_ptr(), ntl, M, COUT, dev["gamma"].data_ptr(),
                 dev["invstd"].data_ptr(), dg.data_ptr(), db.data_ptr(), coef.data_ptr(), S())
            torch.cuda.synchronize()
            yr = y64.clone().requires_grad_(True)
            gr, br = bn["gamma"].double().requires_grad_(True), bn["beta"].double().requires_grad_(True)
            zz = F.batch_norm(yr.t().reshape(1, COUT, M), None, None, gr, br, True, 0.1, 1e-5).reshape(COUT, M).t()
            (F.relu(zz) if bact == 1 else F.hardtanh(zz, 0, 6) if bact == 2 else zz).backward(got.double())
            worst.check("seg_bn_bwd_finalize_tiles", rel(dg, gr.grad), 1e-4, f"case {case} bact {bact} dgamma")
            worst.check("seg_bn_bwd_finalize_tiles", rel(db, br.grad), 1e-4, f"case {case} bact {bact} dbeta")
    worst.write(record)


# ---- seg_conv_igemm_*_ic: split-K combined inside the launch, the tile as an argument -----------------------------

@pytest.mark.parametrize("name", sorted(MATH))
def test_conv_ic(tile, name):
    case = "a"
    job = Job(case, F32)
    splits = splits_for(case)
    for act in (1, 2):
        ref = act_launch(name, job, act, splits)  # the two-launch form
        cnt = torch.zeros(4 * query("seg_conv_igemm_tiles", M, COUT), device=DEV, dtype=torch.int32)
        assert cnt.numel() == 4 * -(-M // TILES[tile][0]) * -(-COUT // TILES[tile][1])
        work = torch.full((splits * M * COUT,), NAN, device=DEV)
        with unforced():  # the tile comes from the argument alone
            for _ in range(2):
                ob = job.out()
                head = job.head(ob)
                call(name + "_ic", *head, act, work.data_ptr(), splits, tile, cnt.data_ptr(), S())
                assert torch.equal(taken(ob), ref), (act, "in-launch combine != two launches")
        check_epoch_words(cnt.cpu(), 2)
