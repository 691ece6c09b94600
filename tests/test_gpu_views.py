"""GPU: every kernel on the channel-slice views the engine hands it.

The decoder concat is never materialised (seg_amd/engine.py: skip concat by channel-slice writes), so the
consumers of a skip tensor read and write Act(buf, off, ld, C) views with a row stride larger than their
channel count -- and include/segamd.h promises that for every entry point.  Each test here launches an entry
point twice on identical inputs (same packed weights, workspace sizes from the library's queries, fresh zeroed
counters): once on contiguous operands, once with the named operands as views of wider buffers
(tests/view_cases.py), and asserts

  (a) the view result is the contiguous result bit for bit -- BatchNorm / BN-backward tile partials and
      weight-gradient slabs included;
  (b) the columns around every view still hold their fill pattern (NaN around inputs: a kernel that reads them
      as data poisons its output; a finite sentinel around outputs);
  (c) for one case per family, the contiguous result still matches the reference the existing test of that
      entry point uses, at that test's bound (no tolerance is introduced here).

No entry point takes another internal path depending on the row stride, so nothing falls back from (a) to (c).
Views sit at column 0 of a wider buffer (what the production programs have: MobileNetV2UNet's cat1..cat4 at
(C, ld) = (16, 80), (24, 152), (32, 288), (64, 1344), UNet's at (64, 128) ...) and at one 16-byte vector in.
seg_conv_pw takes K <= 32 only, so the thin data gradients 96 / 144 / 192 -> 16 / 24 / 32 that write those slices
run on the implicit GEMM (test_igemm_views, test_bnout_views), as in the engine; seg_conv_pw's own data-gradient
direction (K = 16 / 24 / 32 -> 96 / 144 / 192) is test_pw_dgrad_views.
tests/test_views_covered.py checks that this file covers every (entry point, operand) the engine gives a view.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from view_cases import NAN, SENTINEL, guards_intact, make_view, same_bits  # noqa: E402

from seg_amd import engine  # noqa: E402
from seg_amd._lib import call, query  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
PLACES = ("off0", "off1")  # the view at column 0 of the wider buffer / one 16-byte vector in
NHW = (2, 9, 13)           # M = 234: more than one row tile of every implicit-GEMM tile height, ragged last tile


def S():
    return torch.cuda.current_stream().cuda_stream


def r8(c):
    return (c + 7) & ~7


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def vals(M, C, seed, scale=1.0, shift=0.0):
    """[M][C] fp32 values exactly representable in bf16: one tensor serves every storage type."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, C, generator=g) * scale + shift).to(BF).float()


def vec(C, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(C, generator=g) * scale + shift).to(DEV)


def p(t):
    return t.data_ptr() if t is not None else None


class Ops:
    """The activation operands of one launch: contiguous, or (roles named in `views`: role -> ld) views of
    wider buffers with the fill pattern around them."""

    def __init__(self, views=None, place="off0"):
        self.views, self.place = views or {}, place
        self.made = {}  # role -> (buffer, off, C, fill or None)

    def _make(self, role, data, dtype, fill):
        M, C = data.shape
        if role in self.views:
            off = 0 if self.place == "off0" else 16 // torch.empty(0, dtype=dtype).element_size()
            buf, ptr, _ = make_view(M, C, self.views[role], off, dtype, fill, data)
            self.made[role] = (buf, off, C, fill)
            return ptr, self.views[role]
        buf = data.to(device=DEV, dtype=dtype).contiguous()
        self.made[role] = (buf, 0, C, None)
        return buf.data_ptr(), C

    def inp(self, role, data, dtype):
        """An input operand holding `data` ([M][C]); returns (pointer, row stride)."""
        return self._make(role, data, dtype, NAN)

    def out(self, role, M, C, dtype, init=None):
        """An output operand; `init` ([M][C]): what it holds before the launch (an in-place addend, an
        accumulated gradient)."""
        return self._make(role, torch.full((M, C), SENTINEL) if init is None else init, dtype, SENTINEL)

    def get(self, role):
        buf, off, C, _ = self.made[role]
        return buf[:, off:off + C].contiguous()


def pair(fn, views, place):
    """fn(ops) -> {name: tensor} launches on ops' operands.  Runs it on contiguous operands and on `views`,
    asserts (a) and (b), returns the contiguous run's (Ops, results) for (c)."""
    c, v = Ops(), Ops(views, place)
    rc, rv = fn(c), fn(v)
    torch.cuda.synchronize()
    assert set(views) <= set(v.made) and set(c.made) == set(v.made), (views, list(v.made))
    for role in c.made:
        assert same_bits(c.get(role), v.get(role)), f"operand {role}: the view run differs from the contiguous run"
    assert set(rc) == set(rv)
    for k in rc:
        assert same_bits(rc[k], rv[k]), f"{k}: the view run differs from the contiguous run"
    for role, (buf, off, C, fill) in v.made.items():
        if fill is not None:
            assert guards_intact(buf, off, C, fill), f"operand {role}: columns outside the view were written"
    return c, rc


def pack(w, w16, mode=0):
    """w [Cout][Cin][ks][ks] (device) -> the implicit GEMM's packed weight (fp32, or bf16 for the _w16 entries)."""
    Cout, Cin, ks, _ = w.shape
    ldk = r8(ks * ks * Cin)
    wk = torch.zeros(Cout * ldk, device=DEV, dtype=BF if w16 else F32)
    table, n, blocks = engine.pack_table([(w.data_ptr(), wk.data_ptr(), Cout, Cin, ks, ldk, mode + (16 if w16 else 0),
                                           Cin)], w.device)
    call("seg_pack_batch", table.data_ptr(), n, blocks, S())
    return wk, ldk


def weight(Cout, Cin, ks, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Cout, Cin, ks, ks, generator=g) * (2.0 / (Cin * ks * ks)) ** 0.5).to(DEV)


def conv64(x, w, b, N, H, W, w_bf16):
    """float64 conv of rows x [M][Cin] (pad ks // 2) -> rows [M][Cout]; w_bf16: the weight rounded as the bf16 MFMA
    operand."""
    Cout, Cin, ks, _ = w.shape
    w64 = (w.to(BF) if w_bf16 else w).double().cpu()
    y = F.conv2d(x.double().view(N, H, W, Cin).permute(0, 3, 1, 2), w64, None if b is None else b.double().cpu(),
                 padding=ks // 2)
    return y.permute(0, 2, 3, 1).reshape(N * H * W, Cout)


# ------------------------------------------------------------------------------------------- seg_conv_pw

PW_VIEWS = [(16, 80), (24, 152), (32, 288)]  # (K, ld) of the skip slices MobileNetV2UNet's expand convs read


def _pw(io, o, M, K, N, mode, x, w, add=None):
    dt, v = (BF, 8) if io else (F32, 4)
    ldk = (K + v - 1) // v * v
    wk = torch.zeros(N, ldk, device=DEV, dtype=dt)
    wk[:, :K] = w.to(DEV).to(dt)
    b = vec(N, 3) if mode == "bias_stat" else None
    xs, xb = (vec(K, 4, 0.3, 1.0), vec(K, 5)) if mode == "xf" else (None, None)
    xp, ldx = o.inp("in", x, dt)
    op, ldo = o.out("out", M, N, dt, init=add)
    tiles = query("seg_conv_pw_row_tiles", M)
    stat = torch.full((tiles * 2 * N,), NAN, device=DEV) if mode == "bias_stat" else None
    call("seg_conv_pw_bf16io" if io else "seg_conv_pw", xp, ldx, M, K, wk.data_ptr(), ldk, p(b), op, ldo, N,
         op if add is not None else None, ldo if add is not None else 0, p(stat), p(xs), p(xb),
         2 if mode == "xf" else 0, S())
    return ({"stat": stat} if stat is not None else {}), b, xs, xb


def _pw_ref(io, got, x, w, b, xs, xb, add):
    """tests/test_gpu_pw.py::test_pw_matches_float64's reference and bound."""
    a = x.double()
    if xs is not None:
        a = torch.clamp(a * xs.double().cpu() + xb.double().cpu(), 0, 6)
        a = a.float().to(BF).double() if io else (x * xs.cpu() + xb.cpu()).clamp(0, 6).double()
    ref = a @ w.double().t()
    if b is not None:
        ref = ref + b.double().cpu()
    if add is not None:
        ref = ref + add.double()
    err = (got.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
    assert err <= (2.0 ** -7 if io else 1e-5), err


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("mode", ["plain", "bias_stat", "xf"])
@pytest.mark.parametrize("K,ld", PW_VIEWS)
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
def test_pw_forward_views(io, K, ld, mode, place):
    """The expand convs 16 -> 96, 24 -> 144, 32 -> 192 reading their skip slice; M = 777: seven 128-row tiles, the
    last ragged."""
    M, N = 777, 6 * K
    x, w = vals(M, K, 1, 1.3, 0.2), vals(N, K, 2, 0.2)
    extra = {}

    def fn(o):
        res, *extra["coef"] = _pw(io, o, M, K, N, mode, x, w)
        return res

    c, _ = pair(fn, {"in": ld}, place)
    if place == "off0":
        _pw_ref(io, c.get("out"), x, w, *extra["coef"], None)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("K", [16, 24, 32])
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
def test_pw_dgrad_views(io, K, place):
    """seg_conv_pw as a data gradient (thin dY, K = 16 / 24 / 32 -> 6K channels) writing a slice, the fused addend
    read in place from it (Run.begin_write_add: add == out)."""
    M, N = 777, 6 * K
    x, w, add = vals(M, K, 6), vals(N, K, 7, 0.2), vals(M, N, 8)
    c, _ = pair(lambda o: _pw(io, o, M, K, N, "plain", x, w, add)[0], {"out": N + 56}, place)
    if place == "off0" and K == 16:
        _pw_ref(io, c.get("out"), x, w, None, None, None, add)


# ------------------------------------------------------------------------- seg_conv_igemm and its twins

IGEMM = {  # entry point -> (storage, bf16 operands, bf16 packed weights, lazy-BN input transform)
    "seg_conv_igemm": (F32, False, False, False), "seg_conv_igemm_bf16": (F32, True, False, False),
    "seg_conv_igemm_bf16io": (BF, True, False, False), "seg_conv_igemm_bf16io_w16": (BF, True, True, False),
    "seg_conv_igemm_xf": (F32, False, False, True), "seg_conv_igemm_bf16_xf": (F32, True, False, True),
    "seg_conv_igemm_bf16io_xf": (BF, True, False, True), "seg_conv_igemm_bf16io_xf_w16": (BF, True, True, True),
}
IGEMM_SHAPES = {  # Cin, Cout, ks, views, BN partials, in-place addend
    "fwd64_384": (64, 384, 1, {"in": 1344}, True, False),        # op 30 of MobileNetV2UNet: reads cat4[:, :64]
    "dgrad384_64": (384, 64, 1, {"out": 1344}, False, True),     # its data gradient: into the gradient slice
    "conv3x3": (64, 96, 3, {"in": 1344, "out": 160}, True, False),
    "dgrad96_16": (96, 16, 1, {"out": 80}, False, True),         # ops 3, 9, 18: the thin data gradients
    "dgrad144_24": (144, 24, 1, {"out": 152}, False, True),
    "dgrad192_32": (192, 32, 1, {"out": 288}, False, True),
}


def _igemm(name, o, shape, x, w, add):
    dt, _, w16, xf = IGEMM[name]
    Cin, Cout, ks, _, stat_on, _ = IGEMM_SHAPES[shape]
    N, H, W = NHW
    M = N * H * W
    wk, ldk = pack(w, w16)
    b = vec(Cout, 13) if stat_on else None
    xp, ldx = o.inp("in", x, dt)
    op, ldo = o.out("out", M, Cout, dt, init=add)
    tiles = query("seg_conv_igemm_row_tiles", M, Cout, None)
    stat = torch.full((tiles * 2 * Cout,), NAN, device=DEV) if stat_on else None
    tail = (0, None, 1) if name == "seg_conv_igemm_bf16" else ()  # act, work, splits
    coef = (vec(Cin, 14, 0.3, 1.0), vec(Cin, 15)) if xf else ()
    call(name, xp, ldx, N, H, W, Cin, wk.data_ptr(), ldk, p(b), op, ldo, H, W, Cout, ks, 1, ks // 2,
         op if add is not None else None, ldo if add is not None else 0, p(stat), *tail,
         *((coef[0].data_ptr(), coef[1].data_ptr(), 2) if xf else ()), S())
    return ({"stat": stat} if stat_on else {}), b, coef


def _igemm_ref(name, shape, c, rc, x, w, b, coef, add):
    """(c): f32 / bf16 against float64 of the same operands at 1e-5 (tests/test_gpu_ops.py, test_gpu_bf16.py); the
    bf16io entries bitwise the bf16-math launch on fp32 storage rounded once (tests/test_gpu_bf16io.py), the _w16 ones
    bitwise their fp32-weight twins (tests/test_gpu_w16.py); the lazy-BN twins bitwise seg_bn_apply followed by the
    plain launch (tests/test_gpu_lazy_pw.py)."""
    dt, bf, w16, xf = IGEMM[name]
    N, H, W = NHW
    got = c.get("out")
    if xf:  # x = act(in * scale + shift) stored by the apply pass, then the plain conv
        plain = name.replace("_xf", "")
        M, Cin = x.shape
        xa = torch.zeros(M, Cin, device=DEV, dtype=dt)
        xg = x.to(DEV).to(dt)
        call("seg_bn_apply" + ("_bf16io" if dt == BF else ""), xg.data_ptr(), Cin, M, Cin, coef[0].data_ptr(),
             coef[1].data_ptr(), 2, None, 0, xa.data_ptr(), Cin, S())
        o2 = Ops()
        r2, _, _ = _igemm(plain, o2, shape, xa.float().cpu(), w, add)
        torch.cuda.synchronize()
        assert same_bits(got, o2.get("out")) and all(same_bits(rc[k], r2[k]) for k in rc)
    elif dt == BF:
        twin = "seg_conv_igemm_bf16io" if w16 else "seg_conv_igemm_bf16"
        o2 = Ops()
        r2, _, _ = _igemm(twin, o2, shape, x, w, add)
        torch.cuda.synchronize()
        assert same_bits(got, o2.get("out").to(BF)) and all(same_bits(rc[k], r2[k]) for k in rc)
    else:
        ref = conv64(x, w, b, N, H, W, bf)
        if add is not None:
            ref = ref + add.double()
        assert rel(got, ref) < 1e-5


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("shape", list(IGEMM_SHAPES))
@pytest.mark.parametrize("name", list(IGEMM))
def test_igemm_views(name, shape, place):
    Cin, Cout, ks, views, _, addend = IGEMM_SHAPES[shape]
    M = NHW[0] * NHW[1] * NHW[2]
    x, w = vals(M, Cin, 11, 1.3, 0.2), weight(Cout, Cin, ks, 12)
    add = vals(M, Cout, 16) if addend else None
    extra = {}

    def fn(o):
        res, *extra["b_coef"] = _igemm(name, o, shape, x, w, add)
        return res

    c, rc = pair(fn, views, place)
    if place == "off0" and shape in ("fwd64_384", "dgrad384_64"):
        _igemm_ref(name, shape, c, rc, x, w, *extra["b_coef"], add)


# -------------------------------------------------------------------------------- seg_conv_igemm2_bf16io

def ig2_plan(M, Cout, Cin, ks):
    out = (ctypes.c_long * 4)()
    ok = query("seg_conv_igemm2_plan", M, Cout, Cin, ks, ctypes.addressof(out))
    return ok, list(out)  # tile rows, row tiles, split-K slices, workspace floats


def _split_case():
    """The first split-K shape of tests/test_gpu_igemm2.py's CASES, (N, Cin, Cout, H, W, ks) = (2, 1344, 256, 16, 32,
    3), at the smallest batch N for which the plan still splits."""
    for N in (1, 2):
        ok, (_, _, splits, _) = ig2_plan(N * 16 * 32, 256, 1344, 3)
        if ok and splits > 1:
            return N
    raise AssertionError("seg_conv_igemm2_plan no longer splits (2, 1344, 256, 16, 32, 3)")


IG2_SHAPES = {  # N (None: _split_case), H, W, Cin, Cout, ks, views, BN partials, in-place addend
    "fwd64_384": (NHW[0], NHW[1], NHW[2], 64, 384, 1, {"in": 1344}, True, False),
    "dgrad384_64": (NHW[0], NHW[1], NHW[2], 384, 64, 1, {"out": 1344}, False, True),
    "splitk3x3": (None, 16, 32, 1344, 256, 3, {"in": 1344 + 64, "out": 512}, True, False),
}


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("shape", list(IG2_SHAPES))
def test_igemm2_views(shape, place):
    N, H, W, Cin, Cout, ks, views, stat_on, addend = IG2_SHAPES[shape]
    N = N or _split_case()
    M = N * H * W
    ok, (tile_rows, ntiles, splits, work_floats) = ig2_plan(M, Cout, Cin, ks)
    assert ok, "the plan must apply to these shapes"
    assert splits > 1 or shape != "splitk3x3"
    x, w = vals(M, Cin, 21, 1.3, 0.2), weight(Cout, Cin, ks, 22)
    add = vals(M, Cout, 23) if addend else None
    wk, ldk = pack(w, True)
    b = vec(Cout, 24) if stat_on else None

    def fn(o):
        xp, ldx = o.inp("in", x, BF)
        op, ldo = o.out("out", M, Cout, BF, init=add)
        work = torch.zeros(max(work_floats, 1), device=DEV)  # tickets: zero before the first use
        stat = torch.full((ntiles * 2 * Cout,), NAN, device=DEV) if stat_on else None
        call("seg_conv_igemm2_bf16io", xp, ldx, N, H, W, Cin, wk.data_ptr(), ldk, p(b), op, ldo, Cout, ks,
             op if addend else None, ldo if addend else 0, p(stat), work.data_ptr(), S())
        return {"stat": stat} if stat_on else {}

    c, rc = pair(fn, views, place)
    if place == "off0":  # tests/test_gpu_igemm2.py: float64 of the same bf16 operands, the stored output's rounding
        ref = conv64(x, w, b, N, H, W, True)
        assert rel(c.get("out").float(), ref + (add.double() if addend else 0)) < 4e-3
        if stat_on:
            assert rel(rc["stat"].view(ntiles, 2, Cout)[:, 0].double().sum(0), ref.sum(0)) < 1e-5


# ----------------------------------------------------------------------------------- seg_conv_igemm_bnout*

BNOUT = {"seg_conv_igemm_bnout": (F32, False), "seg_conv_igemm_bnout_bf16io": (BF, False),
         "seg_conv_igemm_bnout_bf16io_w16": (BF, True)}
BNOUT_SHAPES = [(96, 16, 80), (144, 24, 152), (192, 32, 288), (384, 64, 1344)]  # dY channels, slice (C, ld)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("Cin,Cout,ld", BNOUT_SHAPES)
@pytest.mark.parametrize("name", list(BNOUT))
def test_bnout_views(name, Cin, Cout, ld, place):
    """The data gradients of ops 3 / 9 / 18 / 30 (ConvOp._dgrad on the default path): `out` the gradient slice with
    the addend read in place, `by` (the BN layer's pre-BN output) a view of another wide buffer; the BN-backward tile
    partials bitwise too."""
    dt, w16 = BNOUT[name]
    N, H, W = NHW
    M = N * H * W
    assert query("seg_conv_igemm_bnout_ok", M, Cout, int(dt == BF)), "the picked tile has no per-lane column vector"
    x, w, add, y = vals(M, Cin, 31), weight(Cout, Cin, 1, 32), vals(M, Cout, 33), vals(M, Cout, 34, 2.0)
    wk, ldk = pack(w, w16)
    mean, invstd, gamma = vec(Cout, 35, 0.3), vec(Cout, 36, 0.1, 1.0).abs(), vec(Cout, 37, 0.1, 1.0).abs()
    scale = gamma * invstd
    shift = vec(Cout, 38, 0.2) - mean * scale
    tiles = query("seg_conv_igemm_row_tiles", M, Cout, None)
    act = 2

    def fn(o):
        xp, ldx = o.inp("in", x, dt)
        yp, ldy = o.inp("by", y, dt)
        op, ldo = o.out("out", M, Cout, dt, init=add)
        part = torch.full((tiles * 2 * Cout,), NAN, device=DEV)
        call(name, xp, ldx, N, H, W, Cin, wk.data_ptr(), ldk, op, ldo, Cout, 1, op, ldo, yp, ldy, scale.data_ptr(),
             shift.data_ptr(), mean.data_ptr(), act, part.data_ptr(), S())
        return {"bpart": part}

    c, rc = pair(fn, {"out": ld, "by": ld + 64}, place)
    if place == "off0":  # tests/test_gpu_bnout.py: the plain launch's output bitwise, coefficients vs seg_bn_bwd_coef
        plain = name.replace("_bnout", "")
        xg, ag, yg = x.to(DEV).to(dt), add.to(DEV).to(dt), y.to(DEV).to(dt)
        call(plain, xg.data_ptr(), Cin, N, H, W, Cin, wk.data_ptr(), ldk, None, ag.data_ptr(), Cout, H, W, Cout, 1, 1,
             0, ag.data_ptr(), Cout, None, S())
        assert same_bits(c.get("out"), ag)
        coef, dg, db = (torch.full((n,), NAN, device=DEV) for n in (3 * Cout, Cout, Cout))
        call("seg_bn_bwd_finalize_tiles", rc["bpart"].data_ptr(), tiles, M, Cout, gamma.data_ptr(), invstd.data_ptr(),
             dg.data_ptr(), db.data_ptr(), coef.data_ptr(), S())
        work = torch.empty(query("seg_chan_workspace_floats", M, Cout), device=DEV)
        coef2, dg2, db2 = (torch.empty(n, device=DEV) for n in (3 * Cout, Cout, Cout))
        call("seg_bn_bwd_coef" + ("_bf16io" if dt == BF else ""), ag.data_ptr(), Cout, yg.data_ptr(), Cout, M, Cout,
             gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), act,
             dg2.data_ptr(), db2.data_ptr(), work.data_ptr(), coef2.data_ptr(), S())
        torch.cuda.synchronize()
        for a, b in ((coef, coef2), (dg, dg2), (db, db2)):
            assert rel(a, b) < 1e-5, rel(a, b)


# ------------------------------------------------------------------------------------------ weight gradients

WGRAD = {  # entry point -> (storage, bf16 operands, lazy-BN input transform)
    "seg_conv_wgrad": (F32, False, False), "seg_conv_wgrad_bf16": (F32, True, False),
    "seg_conv_wgrad_bf16io": (BF, True, False), "seg_conv_wgrad_xf": (F32, False, True),
    "seg_conv_wgrad_bf16_xf": (F32, True, True), "seg_conv_wgrad_bf16io_xf": (BF, True, True),
}
WGRAD_SHAPES = {  # Cin, Cout, ks, views
    "x16_80": (16, 96, 1, {"x": 80}), "x64_1344": (64, 384, 1, {"x": 1344}),
    "x_and_dy": (64, 384, 1, {"x": 1344, "dy": 384 + 64}), "conv3x3": (64, 32, 3, {"x": 128, "dy": 96}),
}


def _wgrad(name, o, Cin, Cout, ks, x, dy, coef):
    dt, bf, xf = WGRAD[name]
    N, H, W = NHW
    M = N * H * W
    splits = query("seg_conv_wgrad_splits_bf16" if bf else "seg_conv_wgrad_splits", M, Cout, Cin, ks)
    dp, lddy = o.inp("dy", dy, dt)
    xp, ldx = o.inp("x", x, dt)
    part = torch.full((splits * Cout * ks * ks * Cin,), NAN, device=DEV)
    call(name, dp, lddy, xp, ldx, N, H, W, Cin, H, W, Cout, ks, 1, ks // 2, part.data_ptr(), splits,
         *((coef[0].data_ptr(), coef[1].data_ptr(), 2) if xf else ()), S())
    return {"part": part}, splits


# (the lazy-BN weight gradient is the 1x1 consumers': Program.make_lazy)
WGRAD_CASES = [(n, s) for n in WGRAD for s in WGRAD_SHAPES if not (WGRAD[n][2] and WGRAD_SHAPES[s][2] == 3)]


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name,shape", WGRAD_CASES)
def test_wgrad_views(name, shape, place):
    """ConvOp._param_grads: x read through the skip slice (rt.ptr(i), i.ld), dY contiguous -- and once a view too."""
    dt, bf, xf = WGRAD[name]
    Cin, Cout, ks, views = WGRAD_SHAPES[shape]
    N, H, W = NHW
    M = N * H * W
    x, dy = vals(M, Cin, 41, 1.3, 0.2), vals(M, Cout, 42)
    coef = (vec(Cin, 43, 0.3, 1.0), vec(Cin, 44)) if xf else None
    extra = {}

    def fn(o):
        res, extra["splits"] = _wgrad(name, o, Cin, Cout, ks, x, dy, coef)
        return res

    c, rc = pair(fn, views, place)
    if place != "off0" or shape not in ("x16_80", "conv3x3"):
        return
    if xf:  # tests/test_gpu_lazy_pw.py: bitwise seg_bn_apply followed by the plain weight gradient
        xa = torch.zeros(M, Cin, device=DEV, dtype=dt)
        xg = x.to(DEV).to(dt)
        call("seg_bn_apply" + ("_bf16io" if dt == BF else ""), xg.data_ptr(), Cin, M, Cin, coef[0].data_ptr(),
             coef[1].data_ptr(), 2, None, 0, xa.data_ptr(), Cin, S())
        r2, _ = _wgrad(name.replace("_xf", ""), Ops(), Cin, Cout, ks, xa.float().cpu(), dy, None)
        torch.cuda.synchronize()
        assert same_bits(rc["part"], r2["part"])
    else:  # tests/test_gpu_ops.py, test_gpu_bf16.py: dW against torch at 1e-5 (operands are bf16 values already)
        dw = torch.empty(Cout, Cin, ks, ks, device=DEV)
        call("seg_conv_wgrad_reduce", rc["part"].data_ptr(), extra["splits"], dw.data_ptr(), Cout, Cin, ks, 0, 0, S())
        to = lambda t, C: t.double().view(N, H, W, C).permute(0, 3, 1, 2)  # noqa: E731
        ref = torch.nn.grad.conv2d_weight(to(x, Cin), (Cout, Cin, ks, ks), to(dy, Cout), padding=ks // 2)
        assert rel(dw, ref) < 1e-5


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", ["seg_conv_wgrad2_bf16io", "seg_conv_wino_wgrad", "seg_conv_wino_wgrad16"])
def test_wgrad_3x3_views(name, place):
    """The 3x3 weight-gradient kernels, x and dY both views.  wgrad2: the smallest H % 4 == 0, W % 64 == 0 image, two
    of them (tiles crossing images), ld % 8 == 0 and seg_conv_wgrad2_ok consulted as _pick_wgrad does."""
    if name == "seg_conv_wgrad2_bf16io":
        dt, (N, H, W, Cin, Cout) = BF, (2, 4, 64, 40, 16)
        assert query("seg_conv_wgrad2_ok", N, H, W, Cin, Cout) == 1
        splits = query("seg_conv_wgrad2_blocks", N, H, W)
        n = splits * Cout * 9 * Cin
    else:
        dt, (N, H, W, Cin, Cout) = F32, (2, 10, 14, 64, 32)
        # (the library's split count is 1 for so few tiles: three slabs, as tests/test_gpu_ops.py also forces)
        splits = max(query(name + "_splits", N, H, W, Cin, Cout), 3)
        n = splits * 16 * Cout * Cin
    M = N * H * W
    x, dy = vals(M, Cin, 51), vals(M, Cout, 52)

    def fn(o):
        dp, lddy = o.inp("dy", dy, dt)
        xp, ldx = o.inp("x", x, dt)
        part = torch.full((n,), NAN, device=DEV)
        call(name, dp, lddy, xp, ldx, N, H, W, Cin, Cout, part.data_ptr(), *(() if dt == BF else (splits,)), S())
        return {"part": part}

    c, rc = pair(fn, {"x": Cin + 64, "dy": Cout + 64}, place)
    if place == "off0":  # tests/test_gpu_wgrad2.py, tests/test_gpu_ops.py: dW against float64 at 1e-5
        dw = torch.full((Cout, Cin, 3, 3), NAN, device=DEV)
        if dt == BF:
            call("seg_conv_wgrad_reduce", rc["part"].data_ptr(), splits, dw.data_ptr(), Cout, Cin, 3, 0, 0, S())
        else:
            call("seg_conv_wino_wgrad_reduce", rc["part"].data_ptr(), splits, dw.data_ptr(), Cout, Cin, Cin, 0, S())
        to = lambda t, C: t.double().view(N, H, W, C).permute(0, 3, 1, 2)  # noqa: E731
        ref = torch.nn.grad.conv2d_weight(to(x, Cin), (Cout, Cin, 3, 3), to(dy, Cout), padding=1)
        assert rel(dw, ref) < 1e-5


# ------------------------------------------------------------------------- Winograd and LDS-halo 3x3 convs

def _pack_wino(w, mode, rows, ldk):
    wk = torch.full((16 * rows * ldk,), NAN, device=DEV)
    jobs, nj, nb = engine.pack_table([(w.data_ptr(), wk.data_ptr(), w.shape[0], w.shape[1], 3, ldk, mode, ldk)], DEV)
    call("seg_pack_batch", jobs.data_ptr(), nj, nb, S())
    return wk


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", ["seg_conv_wino", "seg_conv_wino_fused"])
def test_wino_views(name, place):
    """Winograd F(2x2,3x3) forward with bias and BN partials, `in` and `out` views (the current programs give these
    kernels contiguous rows; the header and _pick_conv's src_ld allow a view).  seg_conv_wino_fused_ok is consulted
    with the view's row stride, as _pick_conv does."""
    N, H, W, Cin, Cout = 2, 10, 14, 64, 32  # M = 280: two 256-row BN tiles, the last ragged
    ldin = Cin + 64
    if name == "seg_conv_wino_fused" and not query("seg_conv_wino_fused_ok", N, H, W, ldin):
        pytest.skip(f"seg_conv_wino_fused_ok({N}, {H}, {W}, {ldin}) == 0: the engine takes seg_conv_wino")
    M = N * H * W
    x, w, b = vals(M, Cin, 61), weight(Cout, Cin, 3, 62), vec(Cout, 63)
    U = _pack_wino(w, 3, Cout, Cin)
    nt = query("seg_conv_wino_row_tiles", N, H, W)

    def fn(o):
        xp, ldx = o.inp("in", x, F32)
        op, ldo = o.out("out", M, Cout, F32)
        stat = torch.full((nt * 2 * Cout,), NAN, device=DEV)
        work = torch.full((16 * (M // 4) * Cout,), NAN, device=DEV)
        call(name, xp, ldx, N, H, W, Cin, U.data_ptr(), Cin, b.data_ptr(), op, ldo, Cout, None, 0, stat.data_ptr(),
             *((work.data_ptr(),) if name == "seg_conv_wino" else ()), S())
        return {"stat": stat}

    c, _ = pair(fn, {"in": ldin, "out": Cout + 64}, place)
    if place == "off0":  # tests/test_gpu_ops.py::test_conv_wino_fwd_stats_dgrad
        assert rel(c.get("out"), conv64(x, w, b, N, H, W, False)) < 1e-5


HALO = {"seg_conv_halo": (F32, False), "seg_conv_halo_bf16io": (BF, False), "seg_conv_halo_bf16io_w16": (BF, True)}


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", list(HALO))
def test_halo_views(name, place):
    """The LDS-halo direct conv on the smallest H % 4 == 0, W % 64 == 0 image, two of them (two 256-row tiles)."""
    dt, w16 = HALO[name]
    N, H, W, Cin, Cout = 2, 4, 64, 64, 32
    assert query("seg_conv_halo_ok", N, H, W, Cin, Cout) == 1
    M = N * H * W
    x, w, b, add = vals(M, Cin, 71), weight(Cout, Cin, 3, 72), vec(Cout, 73), vals(M, Cout, 74)
    wk, ldk = pack(w, w16)
    nt = query("seg_conv_halo_row_tiles", N, H, W)

    def fn(o):
        xp, ldx = o.inp("in", x, dt)
        op, ldo = o.out("out", M, Cout, dt, init=add)
        stat = torch.full((nt * 2 * Cout,), NAN, device=DEV)
        call(name, xp, ldx, N, H, W, Cin, wk.data_ptr(), ldk, b.data_ptr(), op, ldo, Cout, op, ldo, stat.data_ptr(),
             S())
        return {"stat": stat}

    c, rc = pair(fn, {"in": Cin + 64, "out": Cout + 64}, place)
    if place != "off0":
        return
    ref = conv64(x, w, b, N, H, W, dt == BF) + add.double()
    got = c.get("out").double().cpu()
    if dt == F32:  # tests/test_gpu_ops.py::test_conv_halo
        assert rel(got, ref) < 1e-5
    else:  # tests/test_gpu_bf16io.py::test_conv_halo_bf16io: one bf16 rounding of the exact result
        assert bool(((got - ref).abs() <= ref.abs() * 2 ** -8 + 1e-6).all())


# ------------------------------------------------------------------------------------------------ resampling

@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("C,ld", [(64, 128), (256, 512)])
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
def test_maxpool_views(io, C, ld, place):
    """UNet's pools read the skip slice of cat3 / cat1 and scatter into the gradient slice of the same layout, as the
    first writer (accumulate 0) or onto an earlier gradient (1).  Ties in the data: the first maximum takes it."""
    dt, sfx = (BF, "_bf16io") if io else (F32, "")
    N, H, W = 2, 6, 10
    g = torch.Generator().manual_seed(C)
    x = torch.randint(0, 3, (N * H * W, C), generator=g).float()
    dy, prev = vals(N * H * W // 4, C, 81), vals(N * H * W, C, 82)

    def fwd(o):
        xp, ldx = o.inp("in", x, dt)
        op, ldo = o.out("out", N * H * W // 4, C, dt)
        call("seg_maxpool2_fwd" + sfx, xp, ldx, N, H, W, C, op, ldo, S())
        return {}

    c, _ = pair(fwd, {"in": ld}, place)
    to = lambda t, h, w: t.view(N, h, w, C).permute(0, 3, 1, 2)  # noqa: E731
    xr = to(x, H, W).clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    y.backward(to(dy, H // 2, W // 2))
    if place == "off0":  # tests/test_gpu_ops.py::test_maxpool_with_ties
        assert torch.equal(c.get("out").float().cpu(), y.detach().permute(0, 2, 3, 1).reshape(-1, C))
    for acc in (0, 1):
        def bwd(o):
            xp, ldx = o.inp("in", x, dt)
            dp, lddy = o.inp("dout", dy, dt)
            ip, ldi = o.out("din", N * H * W, C, dt, init=prev if acc else None)
            call("seg_maxpool2_bwd" + sfx, xp, ldx, dp, lddy, N, H, W, C, ip, ldi, acc, S())
            return {}

        c, _ = pair(bwd, {"in": ld, "din": ld}, place)
        if place == "off0" and not io:
            ref = xr.grad.permute(0, 2, 3, 1).reshape(-1, C) + (prev if acc else 0)
            assert torch.allclose(c.get("din").cpu(), ref, atol=1e-6)


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
def test_upsample_fwd_views(io, place):
    """UpsampleOp.forward: the x2 upsample writes the upper slice of the cat buffer."""
    dt, sfx = (BF, "_bf16io") if io else (F32, "")
    N, H, W, C = 2, 5, 7, 24
    x = vals(N * H * W, C, 91)

    def fn(o):
        xp, ldx = o.inp("in", x, dt)
        op, ldo = o.out("out", N * 4 * H * W, C, dt)
        call("seg_upsample_fwd" + sfx, xp, ldx, N, H, W, C, op, ldo, 2 * H, 2 * W, 0, S())
        return {}

    c, _ = pair(fn, {"in": 152, "out": 152}, place)
    if place == "off0" and not io:  # tests/test_gpu_ops.py::test_upsample
        ref = F.interpolate(x.view(N, H, W, C).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear",
                            align_corners=False)
        assert rel(c.get("out"), ref.permute(0, 2, 3, 1).reshape(-1, C)) < 1e-6


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("nchw", [0, 1])
@pytest.mark.parametrize("io", [False, True], ids=["f32", "bf16io"])
def test_upsample_bwd_views(io, nchw, ac, acc, place):
    """seg_upsample_bwd into a gradient slice, overwriting and accumulating (accumulate = 1: Run.begin_write_accumulate
    for a `low` that already has a gradient), from an NHWC gradient slice and from the NCHW fp32 logits gradient."""
    dt, sfx = (BF, "_bf16io") if io else (F32, "")
    N, H, W, C = 2, 5, 7, 24
    Ho, Wo = 2 * H, 2 * W
    dy, prev = vals(N * Ho * Wo, C, 95), vals(N * H * W, C, 96)
    dyn = dy.view(N, Ho, Wo, C).permute(0, 3, 1, 2).contiguous().to(DEV)  # the same gradient, NCHW fp32

    def fn(o):
        if nchw:
            dp, lddy = dyn.data_ptr(), 0
        else:
            dp, lddy = o.inp("dout", dy, dt)
        ip, ldi = o.out("din", N * H * W, C, dt, init=prev if acc else None)
        call("seg_upsample_bwd" + sfx, dp, lddy, nchw, N, Ho, Wo, C, ip, ldi, H, W, ac, acc, S())
        return {}

    c, _ = pair(fn, {"din": 152} if nchw else {"din": 152, "dout": 152}, place)
    if place == "off0" and not io:  # tests/test_gpu_ops.py::test_upsample (accumulate: + the earlier gradient)
        xr = torch.zeros(N, C, H, W, requires_grad=True)
        F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=bool(ac)).backward(dyn.cpu())
        ref = xr.grad.permute(0, 2, 3, 1).reshape(-1, C) + (prev if acc else 0)
        assert rel(c.get("din"), ref) < 1e-6


# ------------------------------------------------------------------------------------- folded inference forward

def plan_b1(M, Cout, Cin, ks):
    out = (ctypes.c_int * 3)()
    assert query("seg_conv_igemm_plan_b1", M, Cout, Cin, ks, ctypes.addressof(out)) == 0
    return list(out)  # splits, tile, output tiles


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("spin", [-1, 0])
@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split"])
@pytest.mark.parametrize("name", ["seg_conv_igemm_act", "seg_conv_igemm_bf16", "seg_conv_igemm_f16"])
def test_igemm_ic_views(name, split, spin, place):
    """ConvOp.forward_folded: a batch-1 decoder conv (8x16, 1344 -> 256, 3x3: tests/test_gpu_splitk_ic.py's B1) with
    input, output and residual addend views, unsplit and at seg_conv_igemm_plan_b1's split count (the in-launch
    combine writes the view), with the automatic poll bound and with every share handed to the last arrival."""
    H, W, Cin, Cout, ks = 8, 16, 1344, 256, 3
    M = H * W
    splits, tile, ntl = plan_b1(M, Cout, Cin, ks)
    assert splits > 1, "the batch-1 plan no longer splits this conv"
    if not split:
        splits, tile, ntl = 1, -1, query("seg_conv_igemm_tiles", M, Cout)
    ldk = ks * ks * Cin
    g = torch.Generator().manual_seed(101)
    x, add = vals(M, Cin, 102), vals(M, Cout, 103)
    w = (torch.randn(Cout, ldk, generator=g) * 0.05).to(DEV)  # a packed [Cout][K] weight as is
    b = vec(Cout, 104)

    def fn(o):
        xp, ldx = o.inp("in", x, F32)
        ap, lda = o.inp("add", add, F32)
        op, ldo = o.out("out", M, Cout, F32)
        work = torch.full((max(splits * M * Cout, 1),), NAN, device=DEV)
        cnt = torch.zeros(4 * ntl, device=DEV, dtype=torch.int32)
        call(name + "_ic", xp, ldx, 1, H, W, Cin, w.data_ptr(), ldk, b.data_ptr(), op, ldo, H, W, Cout, ks, 1, ks // 2,
             ap, lda, 1, work.data_ptr(), splits, tile, cnt.data_ptr(), S())
        return {}

    call("seg_set_combine_spin", spin)
    try:
        c, _ = pair(fn, {"in": Cin + 64, "out": Cout + 64, "add": Cout + 64}, place)
    finally:
        call("seg_set_combine_spin", -1)
    if place == "off0":  # tests/test_gpu_splitk_ic.py: bitwise the two-launch split-K at the same split count
        xg, ag = x.to(DEV), add.to(DEV)
        ref = torch.empty(M, Cout, device=DEV)
        work = torch.empty(max(splits * M * Cout, 1), device=DEV)
        call(name, xg.data_ptr(), Cin, 1, H, W, Cin, w.data_ptr(), ldk, b.data_ptr(), ref.data_ptr(), Cout, H, W, Cout,
             ks, 1, ks // 2, ag.data_ptr(), Cout, None, 1, work.data_ptr(), splits, S())
        torch.cuda.synchronize()
        assert same_bits(c.get("out"), ref)


def _mbconv_ref(x, we, be, wd, bd, wp, bp, stride, res):
    """tests/test_gpu_mbconv.py's float64 NCHW block with the kernel's rounding points."""
    h16 = lambda t: t.to(torch.float16).double()  # noqa: E731
    h = F.conv2d(h16(x.double()), h16(we)[:, :, None, None]) + be.double()[None, :, None, None]
    h = h.clamp(0, 6).float().double()
    C = h.shape[1]
    d = F.conv2d(h, wd.double().view(C, 1, 3, 3), stride=stride, padding=1, groups=C) + bd.double()[None, :, None, None]
    o = F.conv2d(h16(d.clamp(0, 6)), h16(wp)[:, :, None, None]) + bp.double()[None, :, None, None]
    return o if res is None else o + res.double()


MBCONV = [  # N, H, W, Cin, ld of x, Cout, ld of out (and res), stride, residual -- expand ratio 6
    (1, 13, 21, 16, 80, 24, 152, 2, False), (2, 13, 21, 24, 152, 24, 152, 1, True),
    (1, 11, 19, 32, 288, 64, 1344, 2, False), (1, 9, 10, 64, 1344, 64, 1344, 1, True),
    (1, 64, 72, 16, 80, 24, 152, 1, True),  # 144 tiles: past the block cap, the hidden range stays whole
]


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("N,H,W,Cin,ldx,Cout,ldo,stride,res", MBCONV)
def test_mbconv_views(N, H, W, Cin, ldx, Cout, ldo, stride, res, place):
    """Run._mbconv: the fused inverted residual reads x (and the residual) and writes out through the cat slices;
    the first four cases split the hidden range (the in-launch combine writes the view), the last does not."""
    Ch = 6 * Cin
    assert query("seg_mbconv_ok", Cin, Ch, Cout, stride, 1) == 1
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.Generator().manual_seed(N * H * W + Cin + Cout)
    x = torch.randn(N * H * W, Cin, generator=g)
    we, be = torch.randn(Ch, Cin, generator=g) / Cin ** 0.5, torch.randn(Ch, generator=g) * 0.1 + 0.5
    wd, bd = torch.randn(Ch, 9, generator=g) / 3, torch.randn(Ch, generator=g) * 0.1 + 0.2
    wp, bp = torch.randn(Cout, Ch, generator=g) / Ch ** 0.5, torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(N * Ho * Wo, Cout, generator=g) if res else None
    wdk = torch.empty(9 * Ch, device=DEV)
    call("seg_pack_dw_weight", wd.contiguous().to(DEV).data_ptr(), wdk.data_ptr(), Ch, S())
    weg, beg, bdg, wpg, bpg = (t.to(DEV) for t in (we, be, bd, wp, bp))
    ncnt = ctypes.c_int(0)
    nw = query("seg_mbconv_work_floats", N, H, W, Ch, Cout, stride, ctypes.addressof(ncnt))
    assert (nw > 0) == (H < 64), "which cases split their hidden range changed"

    def fn(o):
        xp, lx = o.inp("x", x, F32)
        rp, lr = o.inp("res", r, F32) if res else (None, 0)
        op, lo = o.out("out", N * Ho * Wo, Cout, F32)
        work = torch.full((max(nw, 1),), NAN, device=DEV)
        cnt = torch.zeros(max(ncnt.value, 1), device=DEV, dtype=torch.int32)
        call("seg_mbconv_f16", xp, lx, N, H, W, Cin, weg.data_ptr(), beg.data_ptr(), Ch, wdk.data_ptr(), bdg.data_ptr(),
             stride, wpg.data_ptr(), bpg.data_ptr(), Cout, rp, lr, op, lo, work.data_ptr(), cnt.data_ptr(), S())
        return {}

    c, _ = pair(fn, {"x": ldx, "out": ldo, **({"res": ldo} if res else {})}, place)
    if place == "off0" and H < 64:  # tests/test_gpu_mbconv.py::test_mbconv_vs_fp64
        to = lambda t, h, w: t.view(N, h, w, -1).permute(0, 3, 1, 2)  # noqa: E731
        ref = _mbconv_ref(to(x, H, W), we, be, wd, bd, wp, bp, stride, to(r, Ho, Wo) if res else None)
        got = to(c.get("out").double().cpu(), Ho, Wo)
        assert float((got - ref).norm() / ref.norm()) < 1e-3


@pytest.mark.parametrize("place", PLACES)
def test_pw2_views(place):
    """Run.forward_folded's head: seg_pw2_f16 reads the last decoder activation through x.ld."""
    M, C2, act = 1000, 10, 1
    g = torch.Generator().manual_seed(111)
    x = torch.randn(M, 32, generator=g)
    w1, b1 = torch.randn(16, 32, generator=g) / 32 ** 0.5, torch.randn(16, generator=g) * 0.1
    w2, b2 = torch.randn(C2, 16, generator=g) / 4, torch.randn(C2, generator=g) * 0.1
    w1g, b1g, w2g, b2g = (t.to(DEV) for t in (w1, b1, w2, b2))

    def fn(o):
        xp, ldx = o.inp("x", x, F32)
        out = torch.full((M, 12), NAN, device=DEV)
        call("seg_pw2_f16", xp, ldx, M, 32, w1g.data_ptr(), b1g.data_ptr(), 16, act, w2g.data_ptr(), b2g.data_ptr(), C2,
             out.data_ptr(), 12, S())
        return {"out": out}

    _, rc = pair(fn, {"x": 288}, place)
    if place == "off0":  # tests/test_gpu_mbconv.py::test_pw2_head_vs_fp64
        h16 = lambda t: t.to(torch.float16).double()  # noqa: E731
        h = (h16(x) @ h16(w1).T + b1.double()).clamp(min=0)
        ref = h.float().to(torch.float16).double() @ h16(w2).T + b2.double()
        assert float((rc["out"][:, :C2].double().cpu() - ref).norm() / ref.norm()) < 1e-4
        assert bool(rc["out"][:, C2:].isnan().all()), "nothing written beyond C2"


@pytest.mark.parametrize("place", PLACES)
def test_stem_pre_views(place):
    """seg_stem_pre_f16 with ldo > Cout (Predictor passes the stem output's o.ld)."""
    import numpy as np
    from seg_amd.infer import MEAN, STD
    (Hf, Wf), (H, W) = (90, 161), (64, 32)
    frame = torch.from_numpy((np.random.default_rng(Hf).random((Hf, Wf, 3)) * 255).astype(np.uint8)).to(DEV)
    g = torch.Generator().manual_seed(Wf)
    wk = (torch.randn(32, 36, generator=g) * 0.3).to(DEV)
    wk.view(32, 9, 4)[:, :, 3] = 0.0  # the padded channel
    b = torch.randn(32, generator=g).to(DEV)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1

    def fn(o):
        op, ldo = o.out("out", Ho * Wo, 32, F32)
        call("seg_stem_pre_f16", frame.data_ptr(), Hf, Wf, frame.stride(0), H, W, *MEAN, *STD, wk.data_ptr(), 36,
             b.data_ptr(), 2, 32, op, ldo, S())
        return {}

    c, _ = pair(fn, {"out": 48}, place)
    if place == "off0":  # tests/test_gpu_mbconv.py::test_stem_pre_equals_preprocess_then_conv
        img = torch.zeros(H * W, 4, device=DEV)
        call("seg_preprocess_bgr", frame.data_ptr(), 1, Hf, Wf, frame.stride(0), img.data_ptr(), 4, H, W, *MEAN, *STD,
             S())
        ref = torch.empty(Ho * Wo, 32, device=DEV)
        call("seg_conv_igemm_f16", img.data_ptr(), 4, 1, H, W, 4, wk.data_ptr(), 36, b.data_ptr(), ref.data_ptr(), 32,
             Ho, Wo, 32, 3, 2, 1, None, 0, None, 2, None, 1, S())
        torch.cuda.synchronize()
        assert float((c.get("out") - ref).norm() / ref.norm()) < 1e-5
