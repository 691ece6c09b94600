"""GPU: seg_bn_frozen_backward[_bf16io] -- the backward through a BatchNorm on frozen (running) statistics, one
pass that writes dY and the affine gradients' partials together.

Operands are channel-slice views (ld > C, off != 0; the columns outside the slice must stay untouched).  The (M, C)
pairs are the smallest that reach every path of the channel reductions' launcher: one block on 4-channel lanes;
two uneven blocks with one lane column; 8-channel lanes; 4-channel lanes forced by the offset; the 512-block cap with
a row tail; a second blockIdx.y slice holding a single lane column.

Bounds.  dY is three fp32 roundings of exact inputs: rtol / atol 1e-6 against fp64 (the figure
tests/test_gpu_bf16io.py uses for the elementwise BatchNorm kernels).  dbeta and the sum inside dgamma: no lane of these
shapes adds more than 17 terms in sequence and 8 in the row-group tree, so the fp32 part of the error is at most
25 * 2^-24 ~ 1.5e-6 of sum |term| (the rest of the reduction is fp64); the bound is that doubled and rounded up,
4e-6 * sum_r |term_r|.  y is drawn so that no z = y*scale + shift lies within 1e-3 of an activation threshold, and
every value is exactly representable in bf16, so the bf16io form sees the same numbers.
"""
import numpy as np
import pytest
import torch

from seg_amd._lib import call, query

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
EPS = float(np.float32(1e-5))
FILL = 7.0
# (M, C, ld, off)
CASES = [(1, 4, 12, 4), (130, 4, 12, 4), (130, 24, 40, 8), (130, 20, 32, 4), (32839, 8, 16, 8), (200, 520, 528, 8)]
NAMES = {torch.float32: "seg_bn_frozen_backward", BF: "seg_bn_frozen_backward_bf16io"}


def S():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """One (M, C, ld, off): bf16-representable operands (fp32 and bf16 twins on the device) and the fp64 reference
    for every activation, computed once."""

    def __init__(self, M, C, ld, off):
        self.M, self.C, self.ld, self.off = M, C, ld, off
        g = torch.Generator().manual_seed(1000 * C + M % 997)
        self.gamma = torch.rand(C, generator=g) + 0.5
        self.beta = torch.randn(C, generator=g) * 0.5
        self.rm = torch.randn(C, generator=g) * 0.2
        self.rv = torch.rand(C, generator=g) + 0.5
        # scale / shift as the engine forms them (seg_bn_eval_coef's fp32 arithmetic)
        inv = 1.0 / torch.sqrt(self.rv + np.float32(1e-5))
        self.scale = self.gamma * inv
        self.shift = self.beta - self.rm * self.gamma * inv
        y = (torch.randn(M, ld, generator=g) * 2.0 + 0.5).to(BF).float()
        sl = slice(off, off + C)
        for _ in range(100):
            z = y[:, sl].double() * self.scale.double() + self.shift.double()
            bad = (z.abs() < 1e-3) | ((z - 6.0).abs() < 1e-3)
            if not bad.any():
                break
            fresh = (torch.randn(M, C, generator=g) * 2.0 + 0.5).to(BF).float()
            y[:, sl] = torch.where(bad, fresh, y[:, sl])
        else:
            raise AssertionError("could not draw y away from the activation thresholds")
        da = torch.randn(M, ld, generator=g).to(BF).float()
        self.y, self.da = y, da
        self.ref = {}
        yv, dv = y[:, sl].double(), da[:, sl].double()
        z = yv * self.scale.double() + self.shift.double()
        for act in (0, 1, 2):
            mask = torch.ones_like(z) if act == 0 else ((z > 0) if act == 1 else ((z > 0) & (z < 6))).double()
            dz = dv * mask
            t = dz * (yv - self.rm.double())
            self.ref[act] = {"dy": dz * self.scale.double(), "dbeta": dz.sum(0), "s": t.sum(0),
                             "abs_dz": dz.abs().sum(0), "abs_t": t.abs().sum(0)}
        self.inv64 = 1.0 / torch.sqrt(self.rv.double() + EPS)
        self.dev = {n: getattr(self, n).to(DEV) for n in ("scale", "shift", "rm", "rv")}
        self.ops = {torch.float32: (y.to(DEV), da.to(DEV)), BF: (y.to(BF).to(DEV), da.to(BF).to(DEV))}

    def run(self, dt, act, affine=True, dy=True):
        """(dgamma, dbeta, dy buffer [M][ld] pre-filled) of one launch; None for what was not asked for."""
        M, C, ld, off = self.M, self.C, self.ld, self.off
        y, da = self.ops[dt]
        d = self.dev
        gw = torch.full((C,), FILL, device=DEV) if affine else None
        gb = torch.full((C,), FILL, device=DEV) if affine else None
        work = torch.empty(query("seg_chan_workspace_floats", M, C), device=DEV) if affine else None
        out = torch.full((M, ld), FILL, device=DEV, dtype=dt) if dy else None
        p = lambda t: t[:, off:].data_ptr()  # noqa: E731
        call(NAMES[dt], p(da), ld, p(y), ld, M, C, d["scale"].data_ptr(), d["shift"].data_ptr(), d["rm"].data_ptr(),
             d["rv"].data_ptr(), EPS, act, gw.data_ptr() if affine else None, gb.data_ptr() if affine else None,
             work.data_ptr() if affine else None, p(out) if dy else None, ld if dy else 0, S())
        return gw, gb, out


_CASES = {}


@pytest.fixture(params=CASES, ids=lambda c: "M%d-C%d-ld%d-off%d" % c)
def case(request):
    key = request.param
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


def outside_untouched(c, buf):
    keep = torch.ones(c.ld, dtype=torch.bool)
    keep[c.off:c.off + c.C] = False
    return bool((buf[:, keep.to(DEV)].float() == FILL).all())


@pytest.mark.parametrize("act", [0, 1, 2])
def test_against_fp64(case, act):
    c, ref = case, case.ref[act]
    gw, gb, dy = c.run(torch.float32, act)
    torch.cuda.synchronize()
    sl = slice(c.off, c.off + c.C)
    got = dy[:, sl].double().cpu()
    print(f"dY max abs err {(got - ref['dy']).abs().max().item():.3g}")
    torch.testing.assert_close(got, ref["dy"], rtol=1e-6, atol=1e-6)
    assert outside_untouched(c, dy)
    eb = (gb.double().cpu() - ref["dbeta"]).abs()
    es = (gw.double().cpu() / c.inv64 - ref["s"]).abs()
    print(f"dbeta err / sum|term| {(eb / ref['abs_dz'].clamp(min=1e-30)).max().item():.3g}, "
          f"dgamma sum err / sum|term| {(es / ref['abs_t'].clamp(min=1e-30)).max().item():.3g}")
    assert bool((eb <= 4e-6 * ref["abs_dz"]).all())
    assert bool((es <= 4e-6 * ref["abs_t"]).all())


@pytest.mark.parametrize("act", [0, 2])
def test_bf16io_twin_null_forms_and_repeat(case, act):
    c = case
    gw, gb, dy = c.run(torch.float32, act)
    gw2, gb2, dy2 = c.run(torch.float32, act)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2) and torch.equal(dy, dy2)  # run to run
    hw, hb, hy = c.run(BF, act)
    hw2, hb2, hy2 = c.run(BF, act)
    assert torch.equal(hw, hw2) and torch.equal(hb, hb2) and torch.equal(hy.view(torch.int16), hy2.view(torch.int16))
    # bf16io on the same bf16-representable data: the same sums, dY after one bf16 rounding
    assert torch.equal(gw, hw) and torch.equal(gb, hb)
    assert torch.equal(hy.view(torch.int16), dy.to(BF).view(torch.int16))
    assert outside_untouched(c, hy)
    for dt, full_w, full_b, full_y in ((torch.float32, gw, gb, dy), (BF, hw, hb, hy)):
        # no affine gradients: the elementwise pass alone, the same dY
        _, _, ey = c.run(dt, act, affine=False)
        assert torch.equal(ey.view(torch.int16 if dt is BF else torch.int32),
                           full_y.view(torch.int16 if dt is BF else torch.int32))
        # no dY: the same affine gradients
        nw, nb, _ = c.run(dt, act, dy=False)
        assert torch.equal(nw, full_w) and torch.equal(nb, full_b)
    # ... which for fp32 is seg_bn_eval_backward's result
    M, C, ld, off = c.M, c.C, c.ld, c.off
    y, da = c.ops[torch.float32]
    ev = torch.full((M, ld), FILL, device=DEV)
    p = lambda t: t[:, off:].data_ptr()  # noqa: E731
    call("seg_bn_eval_backward", p(da), ld, p(y), ld, M, C, c.dev["scale"].data_ptr(), c.dev["shift"].data_ptr(), act,
         p(ev), ld, S())
    assert torch.equal(ev, dy)
