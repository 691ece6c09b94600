"""GPU: the Winograd kernels (csrc/wino.hip) per variant, slab and BN row tile against float64 -- the kernels behind
every dense 3x3 conv with Cin, Cout >= 128 of the fp32 programs (src/unet.py:58,61: forward and data gradient through
seg_conv_wino / seg_conv_wino_fused) and the weight gradient of every stride-1 3x3 conv with Cin, Cout >= 32
(seg_conv_wino_wgrad16, with seg_conv_wino_wgrad as its fallback).

One geometry serves everything: N = 3, H = W = 14.  th = tw = 7, 49 tiles per image, T = 147 = 128 + 19 tiles,
M = 588 = 2 * 256 + 76 pixels.  The image boundaries fall at tiles 49 and 98, inside the first 128-tile block and
mid-wave; tw = 7 is below both K-strip widths of wino_wgrad16_kernel (8 and 16), so its tile cursor wraps more than
one tile row per step and crosses images; the second 128-tile block holds 19 tiles, so the fused kernel's wave pair
(2, 3) has a BN row tile past T and must write nothing; there are three BN row tiles of 64, 64 and 19 tiles.  One
degenerate geometry, N = 5, H = W = 2 (every 4x4 patch is mostly padding), runs at one channel pair per entry point.

References are float64 of the same operands, written here from the matrices of wino.hip's header comment
(B^T, G, A^T below); in float64 they reproduce conv2d / conv2d_input / conv2d_weight (asserted at 1e-12 where each
reference is built).  Evaluated in float32 the same formulas stay at or below 4e-7 rel-L2 at these shapes, so the
project's fp32-accumulation bound, rel-L2 1e-5 (TOL32 of tests/test_gpu_igemm_tiles.py), stands with about 25x room
from the reference alone; it is the only bound used here.

Operands are the channel-slice views the engine hands over: in / x at column 8 of a (C + 16)-column buffer with
finite neighbours; out, add and dY at non-zero offsets of wider buffers that are NaN outside the slice (the out
buffer must still be NaN there after every launch); U packed with ldk = Cin + 4 and its pad columns overwritten with
NaN after seg_pack_batch; work, stat and part NaN before each launch.

Forward / data gradient (test_fwd_dgrad): per case and entry point the forward with bias + BN partials (pack mode 3)
and the data gradient with a view addend and no bias (pack mode 4; the case's (Cin, Cout) are the kernel's K and
output channels in both) against float64 over the whole output and over each BN row tile's pixels on its own; the
same call again gives the same bits; the [row tile][2][Cout] partials tile by tile (sum, and the sum of squared
deviations about the tile mean) against float64 over the kernel's own stored rows of that tile -- row tile r holds
the 2x2 tiles 64 r ... 64 r + 63, i.e. their 4 pixels each, the last one ragged; seg_bn_stats_tiles of those partials
(mean, invstd, running mean, running unbiased variance); and every argument the entry point refuses returns non-zero
and leaves out, stat and work all NaN.

Weight gradient (test_wgrad_slabs): per case and split count every slab of seg_conv_wino_wgrad and
seg_conv_wino_wgrad16, and every one of its 16 transform points on its own, against the float64 partial sum
sum_t (A dY_t A^T)[xi] (x) (B^T X_t B)[xi] over exactly the tile range include/segamd.h promises,
[s * kchunk, min(T, (s + 1) * kchunk)) with kchunk from seg_conv_wino_geometry -- the reduce maps the 16 points to 9
taps, so a 7-dimensional space of slab errors per (co, ci) is invisible in dW; empty splits all zero, no NaN left;
wgrad16's slabs equal the per-point kernel's bitwise up to the sign of zero; the same call twice gives the same bits;
seg_conv_wino_wgrad_reduce on a copy of the slabs (above 16 splits it consumes them): accumulate 0 into a NaN dW,
then accumulate 1 gives twice the gradient, against float64 conv2d_weight.  One case has real Cin = 70 in a
72-padded x (pad channels zero, as the engine pads) and a NaN guard block behind dW that must survive.

test_wino_wgrad_reduce_direct: the reduce alone on synthetic slabs at the split counts production uses and the ends
of its fold path (fold runs of L = 1, 1, 2, 3, 11, 32, 64 slabs).

tests/test_wino_geometry.py (CPU) imports CASES / covered() and pins the production programs' Winograd routes inside
what runs here.
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
TOL = 1e-5  # fp32 accumulation: TOL32 of tests/test_gpu_igemm_tiles.py
SPLITS = (1, 3, 7, 40)          # at T = 147: kchunk 160, 64, 32, 16 -> 1, 3, 5, 10 filled splits
REDUCE_SPLITS = (1, 16, 17, 40, 169, 512, 1024)
REDUCE_SHAPES = ((12, 10, 12), (32, 32, 32))  # Cout, Cin, Cin_pad
OFF_I, OFF_O, OFF_A, OFF_Y = 8, 8, 16, 8      # column of the in / out / add / dY slice in its buffer

BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)

CASES = {
    # forward / data gradient: (Cin, Cout) -> the template seg_conv_wino's GEMM lands on (seg_conv_wino_fused has one)
    "conv": {
        (40, 72): "128x64",     # Cin = 32 + 8: partial BK-32 chunk; Cout = 64 + 8: partial column tile, and the out
                                # kernel's second channel block has 2 of 16 lanes live
        (72, 136): "128x128",   # second column tile partial
        (40, 392): "128x256",   # 8 waves; 256 + 136: one wave column half out, one fully out
        (40, 256): "128x256",   # production's Cout
        (12, 72): "128x64",     # fused: Cin = 8 + 4, the upper lane half masked in the second K chunk; Cout 2 * 32 + 8
        (152, 64): "128x64",    # fused: production forward
        (64, 152): "128x128",   # fused: production data gradient
    },
    # weight gradient: (Cin, Cout, real Cin) -> (tile of seg_conv_wino_wgrad, tile of seg_conv_wino_wgrad16)
    "wgrad": {
        (136, 136, 136): ("128x128", "64x64"),  # the 64 tile ragged on both sides
        (72, 136, 72): ("128x64", "32x32"),
        (136, 72, 136): ("64x128", "32x32"),
        (72, 72, 72): ("64x64", "32x32"),       # wino_wgrad_kernel<64, 64, 32, 32>: launched by no other test
        (72, 72, 70): ("64x64", "32x32"),       # real Cin = 70 in a 72-padded x
        (136, 40, 136): ("32x128", "32x32"),
        (12, 32, 12): ("32x128", "32x32"),
    },
}
DEGENERATE = {"seg_conv_wino": (40, 72), "seg_conv_wino_fused": (12, 72), "wgrad": (72, 72, 72)}
FUSED_TILE = "128x32"


def covered():
    """({(entry point, variant)} this file compares with float64, the split counts of the reduce test)."""
    out = {("seg_conv_wino", v) for v in CASES["conv"].values()} | {("seg_conv_wino_fused", FUSED_TILE)}
    for pp, ap in CASES["wgrad"].values():
        out |= {("seg_conv_wino_wgrad", pp), ("seg_conv_wino_wgrad16", ap)}
    return out, REDUCE_SPLITS


def S():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def gen(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Geo:
    """N x H x W images as 2x2 output tiles in (n, tile row, tile column) order."""

    def __init__(self, N, H, W):
        self.N, self.H, self.W, self.th, self.tw = N, H, W, H // 2, W // 2
        self.T, self.M = N * self.th * self.tw, N * H * W
        t = torch.arange(self.T)
        n, r = t // (self.th * self.tw), t % (self.th * self.tw)
        ty, tx = r // self.tw, r % self.tw
        # NHWC row of pixel (u, v) of tile t: [T][4]
        self.pix = torch.stack([(n * H + 2 * ty + u) * W + 2 * tx + v for u in (0, 1) for v in (0, 1)], 1)
        self.key = (N, H, W)

    def patches(self, rows):
        """float64 4x4 input patches (pad 1) of NHWC rows [M][C]: [T][C][4][4]."""
        C = rows.shape[1]
        x = F.pad(rows.double().view(self.N, self.H, self.W, C).permute(0, 3, 1, 2), (1, 1, 1, 1))
        p = x.unfold(2, 4, 2).unfold(3, 4, 2)  # [N][C][th][tw][4][4]
        return p.permute(0, 2, 3, 1, 4, 5).reshape(self.T, C, 4, 4)

    def tiles(self, rows):
        """float64 2x2 tiles of NHWC rows [M][C]: [T][C][2][2]."""
        return rows.double()[self.pix].permute(0, 2, 1).reshape(self.T, rows.shape[1], 2, 2)

    def rows(self, y):
        """NHWC rows [M][C] of 2x2 tiles [T][C][2][2]."""
        out = torch.empty(self.M, y.shape[1], dtype=y.dtype)
        out[self.pix.reshape(-1)] = y.permute(0, 2, 3, 1).reshape(self.T * 4, y.shape[1])
        return out

    def nchw(self, rows):
        return rows.double().view(self.N, self.H, self.W, -1).permute(0, 3, 1, 2)

    def row_tile(self, r):
        """NHWC rows of BN row tile r: the pixels of tiles [64 r, min(T, 64 r + 64))."""
        return self.pix[64 * r:min(self.T, 64 * r + 64)].reshape(-1)

    def geometry(self, cin, cout, splits=1, ld=4):
        out = (ctypes.c_int * 6)()
        assert query("seg_conv_wino_geometry", self.N, self.H, self.W, cin, cout, splits, ld,
                     ctypes.addressof(out)) == 0
        return dict(gemm=f"128x{out[0]}", wgrad=f"{out[1]}x{out[2]}", wgrad16=f"{out[3]}x{out[3]}", kchunk=out[4],
                    fallback=out[5])


GEO = Geo(3, 14, 14)
TINY = Geo(5, 2, 2)
assert (GEO.T, GEO.M) == (147, 588)


def wino_conv64(geo, rows, w):
    """float64 Y = A^T [sum_ci (G g G^T) .* (B^T d B)] A of NHWC rows [M][K] and w [C][K][3][3], as rows [M][C]."""
    v = torch.einsum("ip,tcpq,jq->tcij", BT, geo.patches(rows), BT)
    u = torch.einsum("ip,ocpq,jq->ocij", G, w.double(), G)
    m = torch.einsum("tcij,ocij->toij", v, u)
    return geo.rows(torch.einsum("ip,topq,jq->toij", AT, m, AT))


def wino_points64(geo, x, dy):
    """float64 (A dY_t A^T) [T][Cout][4][4] and (B^T X_t B) [T][Cin][4][4] of NHWC rows dy, x."""
    return (torch.einsum("pi,tcpq,qj->tcij", AT, geo.tiles(dy), AT),
            torch.einsum("ip,tcpq,jq->tcij", BT, geo.patches(x), BT))


class Worst:
    """The largest error / bound ratio per (entry point, variant) of one test, for the parity record."""

    def __init__(self, case):
        self.case, self.m, self.t0 = case, {}, time.perf_counter()

    def check(self, name, variant, err, what):
        self.m[name, variant] = max(self.m.get((name, variant), 0.0), err / TOL)
        print(f"{name} {variant} {self.case} {what}: {err:.3e} (bound {TOL:g})")
        assert err < TOL, (name, variant, self.case, what, err)

    def write(self, record):
        sec = time.perf_counter() - self.t0
        for (name, variant), m in self.m.items():
            record(entry=name, variant=variant, case=str(self.case), worst_margin=m, test_seconds=sec)


def all_nan(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in ts)


# ---- forward and data gradient -----------------------------------------------------------------------------------

_CONV = {}


def conv_data(geo, K, C):
    """Operands and float64 references of one (geometry, Cin = K, Cout = C): once, shared by both entry points."""
    key = (geo.key, K, C)
    if key not in _CONV:
        k = 1000 * K + C
        x, dy = gen(geo.M, K, seed=k + 1), gen(geo.M, K, seed=k + 2)
        wf = gen(C, K, 3, 3, seed=k + 3) * (2.0 / (9 * K)) ** 0.5  # forward: K -> C
        wd = gen(K, C, 3, 3, seed=k + 4) * (2.0 / (9 * K)) ** 0.5  # data gradient of a C -> K conv
        b, add = gen(C, seed=k + 5), gen(geo.M, C, seed=k + 6)
        fwd = wino_conv64(geo, x, wf) + b.double()
        dgr = wino_conv64(geo, dy, wd.transpose(0, 1).flip(2, 3)) + add.double()
        # the formulas above are the convolution
        y = F.conv2d(geo.nchw(x), wf.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(geo.M, C)
        dx = torch.nn.grad.conv2d_input((geo.N, C, geo.H, geo.W), wd.double(), geo.nchw(dy), padding=1)
        assert rel(fwd, y) < 1e-12 and rel(dgr, dx.permute(0, 2, 3, 1).reshape(geo.M, C) + add.double()) < 1e-12
        _CONV[key] = dict(x=x, dy=dy, wf=wf, wd=wd, b=b, add=add, fwd=fwd, dgr=dgr)
    return _CONV[key]


def pack_u(w, mode, rows, K):
    """U [16][rows][ldk = K + 4] of seg_pack_batch mode 3 / 4, its pad columns NaN."""
    from seg_amd.engine import pack_table
    ldk = K + 4
    wk = torch.full((16, rows, ldk), NAN, device=DEV)
    table, n, blocks = pack_table([(w.data_ptr(), wk.data_ptr(), w.shape[0], w.shape[1], 3, ldk, mode, ldk)], DEV)
    call("seg_pack_batch", table.data_ptr(), n, blocks, S())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(wk).any())
    wk[:, :, K:] = NAN
    return wk, ldk


class ConvJob:
    """The device operands of one launch form (pack mode 3: forward, 4: data gradient) as channel-slice views."""

    def __init__(self, geo, K, C, mode, d):
        self.geo, self.K, self.C, self.mode = geo, K, C, mode
        self.ldin, self.ldo, self.lda = K + 16, C + 24, C + 32
        buf = gen(geo.M, self.ldin, seed=7)  # finite neighbours
        buf[:, OFF_I:OFF_I + K] = d["x"] if mode == 3 else d["dy"]
        self.inb = buf.to(DEV)
        self.w = (d["wf"] if mode == 3 else d["wd"]).to(DEV)
        self.wk, self.ldk = pack_u(self.w, mode, C, K)
        self.bias = d["b"].to(DEV) if mode == 3 else None
        self.addb = None
        if mode == 4:
            buf = torch.full((geo.M, self.lda), NAN)
            buf[:, OFF_A:OFF_A + C] = d["add"]
            self.addb = buf.to(DEV)
        self.ntl = query("seg_conv_wino_row_tiles", geo.N, geo.H, geo.W)
        assert self.ntl == -(-geo.T // 64) and query("seg_conv_wino_tile_rows") == 256

    def buffers(self):
        """out (a C-column slice at column OFF_O), stat (one guard row tile behind the ntl the kernels own), work."""
        return (torch.full((self.geo.M, self.ldo), NAN, device=DEV),
                torch.full((self.ntl + 1, 2, self.C), NAN, device=DEV),
                torch.full((16 * self.geo.T * self.C,), NAN, device=DEV))

    def args(self, entry, ob, stat, wbuf, **over):
        g = self.geo
        a = dict(inp=self.inb.data_ptr() + 4 * OFF_I, ldin=self.ldin, N=g.N, H=g.H, W=g.W, Cin=self.K,
                 wk=self.wk.data_ptr(), ldk=self.ldk, bias=self.bias.data_ptr() if self.bias is not None else None,
                 out=ob.data_ptr() + 4 * OFF_O, ldout=self.ldo, Cout=self.C,
                 add=self.addb.data_ptr() + 4 * OFF_A if self.addb is not None else None,
                 ldadd=self.lda if self.addb is not None else 0,
                 stat=stat.data_ptr() if self.mode == 3 else None)
        if entry == "seg_conv_wino":
            a["work"] = wbuf.data_ptr()
        a.update(over)
        return tuple(a.values()) + (S(),)

    def run(self, entry):
        ob, stat, work = self.buffers()
        call(entry, *self.args(entry, ob, stat, work))
        torch.cuda.synchronize()
        o = ob.cpu()
        assert bool(torch.isnan(o[:, :OFF_O]).all()) and bool(torch.isnan(o[:, OFF_O + self.C:]).all()), \
            "a store outside the output slice"
        return o[:, OFF_O:OFF_O + self.C].contiguous(), stat.cpu()

    def refusals(self, entry):
        """Every argument the entry point rejects: non-zero, and nothing launched."""
        g, K, C = self.geo, self.K, self.C
        bad = [dict(H=g.H - 1), dict(W=g.W - 1), dict(Cin=K - 2), dict(Cout=C - 2), dict(ldin=self.ldin + 2),
               dict(ldk=self.ldk + 2), dict(ldk=K - 4)]
        addp = self.inb.data_ptr()  # any non-null addend: the stride is refused before it is read
        if entry == "seg_conv_wino":
            bad += [dict(work=None), dict(ldout=self.ldo + 2), dict(add=addp, ldadd=self.lda + 2)]
        else:
            big_ldk = (-(-(1 << 31) // (64 * C)) + 3) & ~3  # 16 * Cout * ldk * 4 bytes >= 2^31
            big_ldin = 1 << 28                              # the images of one block beyond the 32-bit offsets
            assert query("seg_conv_wino_fused_ok", g.N, g.H, g.W, big_ldin) == 0
            bad += [dict(ldout=C - 4), dict(add=addp, ldadd=C - 4), dict(ldin=big_ldin), dict(ldk=big_ldk)]
        ob, stat, work = self.buffers()
        for over in bad:
            assert query(entry, *self.args(entry, ob, stat, work, **over)) != 0, (entry, over)
        assert all_nan(ob, stat, work), (entry, "a refused call wrote")


def check_conv(worst, entry, variant, job, d):
    geo, C = job.geo, job.C
    what = "fwd" if job.mode == 3 else "dgrad"
    want = d["fwd"] if job.mode == 3 else d["dgr"]
    got, stat = job.run(entry)
    worst.check(entry, variant, rel(got, want), f"{what} vs fp64")
    for r in range(job.ntl):
        rows = geo.row_tile(r)
        worst.check(entry, variant, rel(got[rows], want[rows]), f"{what} row tile {r} vs fp64")
    got2, stat2 = job.run(entry)
    assert torch.equal(got, got2), (entry, what, "not reproducible")
    if job.mode == 4:
        assert bool(torch.isnan(stat).all()), "no BN partials were asked for"
        return
    assert torch.equal(stat[:job.ntl], stat2[:job.ntl]), (entry, "BN partials not reproducible")
    assert bool(torch.isnan(stat[job.ntl]).all()), "a store past the last BN row tile"
    assert not bool(torch.isnan(stat[:job.ntl]).any()), "a BN partial was never written"
    y0 = got.double()
    for r in range(job.ntl):
        blk = y0[geo.row_tile(r)]
        assert blk.shape[0] == 4 * min(64, geo.T - 64 * r)
        worst.check(entry, variant, rel(stat[r, 0], blk.sum(0)), f"tile-sum {r}")
        worst.check(entry, variant, rel(stat[r, 1], ((blk - blk.mean(0)) ** 2).sum(0)), f"tile-M2 {r}")
    st = torch.full((4, C), NAN, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    sd = stat[:job.ntl].contiguous().to(DEV)
    call("seg_bn_stats_tiles", sd.data_ptr(), job.ntl, 256, geo.M, C, None, None, 1e-5, 0.1, rm.data_ptr(),
         rv.data_ptr(), None, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), S())
    torch.cuda.synchronize()
    worst.check("seg_bn_stats_tiles", variant, rel(st[0], y0.mean(0)), "mean")
    worst.check("seg_bn_stats_tiles", variant, rel(st[1], 1 / torch.sqrt(y0.var(0, unbiased=False) + 1e-5)), "invstd")
    worst.check("seg_bn_stats_tiles", variant, rel(rm, 0.1 * y0.mean(0)), "running mean")
    worst.check("seg_bn_stats_tiles", variant, rel(rv, 0.9 + 0.1 * y0.var(0, unbiased=True)), "running var")


def conv_case(entry, geo, K, C, record):
    worst = Worst((geo.key, K, C))
    gemm = geo.geometry(K, C)["gemm"]
    if geo is GEO:
        assert gemm == CASES["conv"][K, C], (K, C, gemm)
    variant = gemm if entry == "seg_conv_wino" else FUSED_TILE
    if entry == "seg_conv_wino_fused":
        assert query("seg_conv_wino_fused_ok", geo.N, geo.H, geo.W, K + 16) == 1
    d = conv_data(geo, K, C)
    for mode in (3, 4):
        job = ConvJob(geo, K, C, mode, d)
        check_conv(worst, entry, variant, job, d)
        job.refusals(entry)
    worst.write(record)


@pytest.mark.parametrize("entry", ["seg_conv_wino", "seg_conv_wino_fused"])
@pytest.mark.parametrize("K,C", sorted(CASES["conv"]), ids=lambda v: str(v))
def test_fwd_dgrad(entry, K, C, record):
    conv_case(entry, GEO, K, C, record)


@pytest.mark.parametrize("entry", ["seg_conv_wino", "seg_conv_wino_fused"])
def test_fwd_dgrad_degenerate(entry, record):
    conv_case(entry, TINY, *DEGENERATE[entry], record)


# ---- weight gradient ---------------------------------------------------------------------------------------------

class WgradJob:
    """x [M][Cin] at column OFF_I of a finite (Cin + 16)-column buffer (channels >= real Cin zero), dY [M][Cout] at
    column OFF_Y of a (Cout + 24)-column buffer that is NaN elsewhere; the float64 points and weight gradient."""

    def __init__(self, geo, cin, cout, creal):
        self.geo, self.cin, self.cout, self.creal = geo, cin, cout, creal
        k = 100000 + 1000 * cin + 10 * cout + (cin - creal)
        x, dy = gen(geo.M, cin, seed=k + 1), gen(geo.M, cout, seed=k + 2)
        x[:, creal:] = 0
        self.ldx, self.lddy = cin + 16, cout + 24
        buf = gen(geo.M, self.ldx, seed=8)
        buf[:, OFF_I:OFF_I + cin] = x
        self.xb = buf.to(DEV)
        buf = torch.full((geo.M, self.lddy), NAN)
        buf[:, OFF_Y:OFF_Y + cout] = dy
        self.dyb = buf.to(DEV)
        self.dyv, self.xv = wino_points64(geo, x, dy)
        self.dw = torch.nn.grad.conv2d_weight(geo.nchw(x[:, :creal]), (cout, creal, 3, 3), geo.nchw(dy), padding=1)
        full = torch.einsum("toij,tcij->ijoc", self.dyv, self.xv)
        # F(3x3, 2x2) is the gradient
        assert rel(torch.einsum("pi,pqoc,qj->ocij", G, full, G)[:, :creal], self.dw) < 1e-12
        self.refs = {}

    def slab_refs(self, kchunk):
        """float64 [16][Cout][Cin] partial of every non-empty split."""
        if kchunk not in self.refs:
            self.refs[kchunk] = [torch.einsum("toij,tcij->ijoc", self.dyv[lo:lo + kchunk], self.xv[lo:lo + kchunk])
                                 .reshape(16, self.cout, self.cin) for lo in range(0, self.geo.T, kchunk)]
        return self.refs[kchunk]

    def launch(self, entry, splits):
        g = self.geo
        part = torch.full((splits, 16, self.cout, self.cin), NAN, device=DEV)
        call(entry, self.dyb.data_ptr() + 4 * OFF_Y, self.lddy, self.xb.data_ptr() + 4 * OFF_I, self.ldx, g.N, g.H,
             g.W, self.cin, self.cout, part.data_ptr(), splits, S())
        torch.cuda.synchronize()
        return part


def check_slabs(worst, entry, variant, part, refs, what):
    p = part.cpu()
    assert not bool(torch.isnan(p).any()), (entry, what, "a slab element was never written")
    filled = len(refs)
    assert filled <= p.shape[0]
    errs = [rel(p[s], refs[s]) for s in range(filled)]
    s = max(range(filled), key=errs.__getitem__)
    worst.check(entry, variant, errs[s], f"{what}: worst of {filled} slabs (slab {s})")
    perr = [(rel(p[s, xi], refs[s][xi]), s, xi) for s in range(filled) for xi in range(16)]
    e, s, xi = max(perr)
    worst.check(entry, variant, e, f"{what}: worst of {16 * filled} points (slab {s} point {xi})")
    for s in range(filled, p.shape[0]):
        assert int(torch.count_nonzero(p[s])) == 0, (entry, what, f"empty split {s} is not all zero")


def check_reduce(worst, job, part, what):
    """seg_conv_wino_wgrad_reduce of a copy of the slabs into a NaN dW, then of another copy on top, against float64;
    dW is followed by a NaN guard block."""
    n = job.cout * job.creal * 9
    dw = torch.full((n + 1024,), NAN, device=DEV)
    for acc in (0, 1):
        p = part.clone()
        call("seg_conv_wino_wgrad_reduce", p.data_ptr(), part.shape[0], dw.data_ptr(), job.cout, job.creal, job.cin,
             acc, S())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw[n:]).all()), "a store behind dW"
        worst.check("seg_conv_wino_wgrad_reduce", "reduce", rel(dw[:n].view_as(job.dw), (1 + acc) * job.dw),
                    f"{what} accumulate {acc}")


def wgrad_case(geo, cin, cout, creal, record):
    worst = Worst((geo.key, cin, cout, creal))
    job = WgradJob(geo, cin, cout, creal)
    for splits in SPLITS:
        q = geo.geometry(cin, cout, splits, max(job.ldx, job.lddy))
        assert q["fallback"] == 0
        if geo is GEO:
            assert (q["wgrad"], q["wgrad16"]) == CASES["wgrad"][cin, cout, creal], (cin, cout, q)
            assert q["kchunk"] == {1: 160, 3: 64, 7: 32, 40: 16}[splits]
        refs = job.slab_refs(q["kchunk"])
        assert len(refs) == -(-geo.T // q["kchunk"])
        parts = {}
        for entry, variant in (("seg_conv_wino_wgrad", q["wgrad"]), ("seg_conv_wino_wgrad16", q["wgrad16"])):
            part = parts[entry] = job.launch(entry, splits)
            check_slabs(worst, entry, variant, part, refs, f"splits {splits} kchunk {q['kchunk']}")
            assert torch.equal(part, job.launch(entry, splits)), (entry, splits, "not reproducible")
        assert torch.equal(parts["seg_conv_wino_wgrad16"], parts["seg_conv_wino_wgrad"]), \
            (splits, "the all-points kernel's slabs differ from the per-point kernel's")
        check_reduce(worst, job, parts["seg_conv_wino_wgrad16"], f"splits {splits}")
    worst.write(record)


@pytest.mark.parametrize("cin,cout,creal", sorted(CASES["wgrad"]), ids=lambda v: str(v))
def test_wgrad_slabs(cin, cout, creal, record):
    wgrad_case(GEO, cin, cout, creal, record)


def test_wgrad_slabs_degenerate(record):
    wgrad_case(TINY, *DEGENERATE["wgrad"], record)


@pytest.mark.parametrize("cout,cin,cin_pad", REDUCE_SHAPES)
def test_wino_wgrad_reduce_direct(cout, cin, cin_pad, record):
    """dW = G^T (sum of the slabs) G on synthetic slabs [splits][16][Cout][Cin_pad] whose pad columns are NaN, at
    1, 16 (no fold), 17 (L = 2), 40 (L = 3), 169 (L = 11, last run of 4 slabs), 512 (L = 32) and 1024 (L = 64) splits:
    a fresh copy per call (above 16 splits the slabs are consumed), bitwise reproducible, accumulate 0 into NaN, then
    1."""
    worst = Worst((cout, cin, cin_pad))
    smax = max(REDUCE_SPLITS)
    slabs = gen(smax, 16, cout, cin_pad, seed=900 + cout)
    slabs[..., cin:] = NAN
    dev = slabs.to(DEV)
    n = cout * cin * 9
    for splits in REDUCE_SPLITS:
        m = slabs[:splits, :, :, :cin].double().sum(0).view(4, 4, cout, cin)
        want = torch.einsum("pi,pqoc,qj->ocij", G, m, G)
        bits = []
        for rep in range(2):
            dw = torch.full((n + 1024,), NAN, device=DEV)
            for acc in (0, 1):
                p = dev[:splits].clone()
                call("seg_conv_wino_wgrad_reduce", p.data_ptr(), splits, dw.data_ptr(), cout, cin, cin_pad, acc, S())
                torch.cuda.synchronize()
                assert bool(torch.isnan(dw[n:]).all()), "a store behind dW"
                if rep == 0:
                    worst.check("seg_conv_wino_wgrad_reduce", "reduce", rel(dw[:n].view_as(want), (1 + acc) * want),
                                f"splits {splits} accumulate {acc}")
            bits.append(dw[:n].clone())
        assert torch.equal(bits[0], bits[1]), (splits, "not reproducible")
    for sp, pad in ((0, cin_pad), (1, cin_pad + 2), (1, cin - 4)):  # refused: nothing launches
        dw = torch.full((n,), NAN, device=DEV)
        assert query("seg_conv_wino_wgrad_reduce", dev.data_ptr(), sp, dw.data_ptr(), cout, cin, pad, 0, S()) != 0, \
            (sp, pad)
        assert all_nan(dw)
    worst.write(record)
