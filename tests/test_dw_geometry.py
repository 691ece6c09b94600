"""CPU: the launch geometry of the depthwise 3x3 kernels (csrc/dwconv.hip) through seg_dw_wgrad_geometry -- the host
query the weight gradient's launch and seg_dw_wgrad_blocks take their numbers from -- and what
tests/test_gpu_dw_matrix.py builds on it: every entry of its case tables lands in the launch class it claims; the
query's invariants over small and production sizes; the arguments the query and the four launches refuse on the host;
every depthwise row of tests/golden/engine_routes.json has the query's row blocks as its `splits` and a launch class
the GPU file runs; and, without a GPU, the GPU file's float64 references and bounds themselves: torch's own fp32
evaluation of every case stays inside the bounds, and seven mutations of the reference (the kernel bugs the GPU file
is there to catch) each break them.

No GPU: the queries are host functions and a refused launch returns before it touches the device."""
import ctypes
import importlib.util
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from seg_amd._lib import query

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_dw_matrix as gpu_file  # noqa: E402  -- tables, references and bounds; its tests are marked gpu

_spec = importlib.util.spec_from_file_location("make_engine_routes", os.path.join(HERE, "golden",
                                                                                  "make_engine_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURE = json.load(open(os.path.join(HERE, "golden", "engine_routes.json")))
CONV, WGRAD = gpu_file.CASES["conv"], gpu_file.CASES["wgrad"]
geometry, out_hw, cdiv, ratio = gpu_file.geometry, gpu_file.out_hw, gpu_file.cdiv, gpu_file.ratio
TW = geometry(1, 1, 1, 4)["tw"]


# ---- the case tables -------------------------------------------------------------------------------------------

def fwd_blocks(case, s):
    N, C, H, W = case
    items = gpu_file.conv_items(N, *out_hw(H, W, s), C, TW)
    return cdiv(items, 256), items % 256


def dgrad_blocks(case, s):
    N, C, H, W = case
    items = gpu_file.conv_items(N, H, W, C, TW)
    return cdiv(items, 256), items % 256


def big_odd_grid(blocks_rem):
    blocks, rem = blocks_rem
    return blocks >= 9 and blocks % 8 != 0 and rem != 0


def wo(case, s):
    return out_hw(case[2], case[3], s)[1]


# class -> (predicate of (case, stride), the strides it must be claimed at)
CONV_PRED = {
    "fwd grid >= 9, not a multiple of 8, partial last block": (lambda c, s: big_odd_grid(fwd_blocks(c, s)), (1, 2)),
    "dgrad grid >= 9, not a multiple of 8, partial last block": (lambda c, s: big_odd_grid(dgrad_blocks(c, s)),
                                                                 (1, 2)),
    "Wo % 4 == 1": (lambda c, s: wo(c, s) % 4 == 1 and wo(c, s) > 4, (1, 2)),
    "Wo % 4 == 2": (lambda c, s: wo(c, s) % 4 == 2 and wo(c, s) > 4, (1, 2)),
    "Wo % 4 == 3": (lambda c, s: wo(c, s) % 4 == 3 and wo(c, s) > 4, (1, 2)),
    "Wo < 4": (lambda c, s: 1 < wo(c, s) < 4, (1, 2)),
    "Wo == 1": (lambda c, s: wo(c, s) == 1, (1, 2)),
    "H == 1": (lambda c, s: c[2] == 1, (1, 2)),
    "H odd, W odd": (lambda c, s: c[2] % 2 == 1 and c[3] % 2 == 1 and c[2] > 1 and c[3] > 1, (2,)),
    "H odd, W even": (lambda c, s: c[2] % 2 == 1 and c[3] % 2 == 0 and c[2] > 1, (2,)),
    "H even, W odd": (lambda c, s: c[2] % 2 == 0 and c[3] % 2 == 1 and c[3] > 1, (2,)),
    "H even, W even": (lambda c, s: c[2] % 2 == 0 and c[3] % 2 == 0, (2,)),
    "dgrad W % 4 != 0": (lambda c, s: c[3] % 4 != 0 and c[3] > 4, (2,)),
    "dgrad W == 1": (lambda c, s: c[3] == 1, (2,)),
    "dgrad W == 2": (lambda c, s: c[3] == 2, (2,)),
    "C == 8": (lambda c, s: c[1] == 8, (1, 2)),
    "C % 8 == 4": (lambda c, s: c[1] % 8 == 4, (1, 2)),
    "C == 960": (lambda c, s: c[1] == 960, (1, 2)),
}


def test_conv_cases_land_where_they_claim():
    assert TW == 4 and geometry(1, 1, 1, 4)["tww"] == 4, "the Wo % 4 classes are those of the strip width"
    assert set(gpu_file.CONV_CLASSES) == set(CONV_PRED)
    for name, claims in gpu_file.CONV_CLASSES.items():
        pred, strides = CONV_PRED[name]
        assert {s for _, s in claims} >= set(strides), (name, "is not claimed at every stride it is asked at")
        for case, s in claims:
            assert case in CONV and s in (1, 2) and pred(case, s), (name, case, s)
    # the W % 4 classes of the stride-2 data gradient between them: 1, 2 and 3
    assert {c[3] % 4 for c, _ in gpu_file.CONV_CLASSES["dgrad W % 4 != 0"]} == {1, 2, 3}
    for case in gpu_file.BIAS_ACT_CASES + gpu_file.TWIN_CASES:
        assert case in CONV and fwd_blocks(case, 1)[0] > 1 and dgrad_blocks(case, 2)[0] > 1, case
    assert len(set(gpu_file.BIAS_ACT_CASES)) == 2
    for (N, C, H, W) in CONV:
        assert N >= 2 or H * W == 1


def test_wgrad_cases_land_where_they_claim():
    got = {}
    for case, claim in WGRAD.items():
        N, C, H, W, s = case
        g = got[case] = geometry(N, *out_hw(H, W, s), C)
        assert claim[:5] == (g["blocks"], g["last"], g["RG"], g["gy"], g["idle"]), (case, claim, g)
        assert claim[5] in (0, 1, 2) and N >= 2
        assert 1 <= g["last"] <= g["spb"] and g["RG"] == 256 // g["TC"]
    for C, RG in ((32, 32), (96, 10), (144, 7), (192, 5)):  # >= 3 row blocks with a ragged last one, per RG
        assert any(c[1] == C and g["RG"] == RG and g["blocks"] >= 3 and g["last"] < g["spb"]
                   for c, g in got.items()), (C, RG)
    assert any(g["blocks"] >= 3 and g["last"] < g["RG"] for g in got.values())
    for s in (1, 2):  # gy = 2 with CG % gy != 0: TC = 33, one idle lane in the last chunk
        assert any(c[4] == s and c[1] == 260 and (g["gy"], g["TC"], g["idle"]) == (2, 33, 1) and g["blocks"] >= 3
                   for c, g in got.items()), s
    for C, gy in ((576, 3), (960, 4)):
        assert any(c[1] == C and g["gy"] == gy and g["blocks"] >= 2 for c, g in got.items()), C
    assert any(g["blocks"] * g["gy"] >= 9 and (g["blocks"] * g["gy"]) % 8 for g in got.values())
    assert any(g["blocks"] == 1 and g["nstrips"] < g["RG"] for g in got.values())
    assert {c[4] for c in got} == {1, 2} and {v[5] for v in WGRAD.values()} == {0, 1, 2}
    assert gpu_file.covered() == {gpu_file.wgrad_class(g["blocks"], g["last"], g["RG"], g["gy"], g["idle"])
                                  for g in got.values()}


# ---- the query -------------------------------------------------------------------------------------------------

SWEEP_HW = ((1, 1), (1, 7), (2, 5), (3, 3), (13, 5), (27, 41), (29, 29), (8, 16), (16, 32), (32, 64), (64, 128),
            (128, 256), (512, 1024))
SWEEP_C = (4, 8, 12, 32, 36, 96, 144, 192, 256, 260, 384, 576, 960, 1280, 2052)


def test_query_sweep():
    for N in (1, 2, 5, 32):
        for Ho, Wo in SWEEP_HW:
            for C in SWEEP_C:
                g = geometry(N, Ho, Wo, C)
                key = (N, Ho, Wo, C, g)
                assert g["blocks"] == query("seg_dw_wgrad_blocks", N, Ho, Wo, C), key
                assert g["blocks"] * g["spb"] >= g["nstrips"] > (g["blocks"] - 1) * g["spb"], key
                assert g["TC"] * g["gy"] >= C // 4 and (g["TC"] - 1) * g["gy"] < C // 4, key
                assert g["RG"] * g["TC"] <= 256 and g["RG"] == 256 // g["TC"] >= 4 and g["TC"] <= 64, key
                assert (g["tww"], g["tw"]) == (4, 4) and g["blocks"] * g["gy"] <= 2048, key


def test_refused_query_writes_nothing():
    out = (ctypes.c_int * 7)(*([-7] * 7))
    for args in ((2, 4, 4, 6), (2, 4, 4, 2), (2, 4, 4, 0), (2, 4, 4, -4), (0, 4, 4, 8), (-1, 4, 4, 8), (2, 0, 4, 8),
                 (2, -3, 4, 8), (2, 4, 0, 8), (2, 4, -1, 8)):
        assert query("seg_dw_wgrad_geometry", *args, ctypes.addressof(out)) == 1, args  # hipErrorInvalidValue
        assert tuple(out) == (-7,) * 7, "a refused query writes nothing"
    assert query("seg_dw_wgrad_geometry", 2, 4, 4, 8, None) == 1


def test_launches_refuse_on_the_host():
    """Non-zero before anything is launched (no GPU here): C % 4, ld % 4, stride 3, one of scale / shift null, a
    stride-1 data gradient whose input and output sizes differ, a null bias, an activation outside 0..2."""
    host = (ctypes.c_float * 16)()
    p = ctypes.addressof(host)  # a non-null pointer that is never read
    fwd = dict(inp=p, ldin=8, N=2, H=4, W=4, C=8, sc=None, sh=None, act=0, wk=p, out=p, ldout=8, Ho=4, Wo=4,
               stride=1, stream=None)
    for over in (dict(C=6), dict(ldin=6), dict(ldout=10), dict(stride=3), dict(stride=0), dict(sc=p), dict(sh=p)):
        assert query("seg_dw_fwd", *{**fwd, **over}.values()) == 1, over
        assert query("seg_dw_fwd_bf16io", *{**fwd, **over}.values()) == 1, over
    dgr = dict(dy=p, lddy=8, N=2, Ho=4, Wo=4, C=8, wk=p, dx=p, lddx=8, H=4, W=4, stride=1, acc=0, stream=None)
    for over in (dict(C=6), dict(lddy=6), dict(lddx=10), dict(stride=3), dict(H=5), dict(W=3), dict(H=8, W=8)):
        assert query("seg_dw_dgrad", *{**dgr, **over}.values()) == 1, over
        assert query("seg_dw_dgrad_bf16io", *{**dgr, **over}.values()) == 1, over
    wgr = dict(dy=p, lddy=8, x=p, ldx=8, N=2, H=4, W=4, C=8, sc=None, sh=None, act=0, Ho=4, Wo=4, stride=1, part=p,
               stream=None)
    for over in (dict(C=6), dict(lddy=6), dict(ldx=10), dict(stride=3), dict(sc=p), dict(sh=p)):
        assert query("seg_dw_wgrad", *{**wgr, **over}.values()) == 1, over
        assert query("seg_dw_wgrad_bf16io", *{**wgr, **over}.values()) == 1, over
    epi = dict(inp=p, ldin=8, N=2, H=4, W=4, C=8, wk=p, bias=p, act=2, out=p, ldout=8, Ho=4, Wo=4, stride=1,
               stream=None)
    for over in (dict(C=6), dict(ldin=6), dict(ldout=10), dict(stride=3), dict(bias=None), dict(act=-1),
                 dict(act=3)):
        assert query("seg_dw_fwd_bias_act", *{**epi, **over}.values()) == 1, over
    assert all(v == 0.0 for v in host)


# ---- the production programs ----------------------------------------------------------------------------------

PROGRAMS = [(arch, N, H, W, m) for arch, N, H, W, maths in gen.PROGRAMS for m in maths
            if any(r["wgrad"] and r["wgrad"]["family"] == "dw" for r in FIXTURE[f"{arch} {N}x{H}x{W} {m}"])]


@pytest.mark.parametrize("arch,N,H,W,math", PROGRAMS, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}" for c in PROGRAMS])
def test_production_rows(arch, N, H, W, math):
    prog = gen.build(arch, N, H, W, math)
    classes, n = gpu_file.covered(), 0
    for row in FIXTURE[f"{arch} {N}x{H}x{W} {math}"]:
        wg = row["wgrad"]
        if not wg or wg["family"] != "dw":
            continue
        n += 1
        op = prog.ops[row["op"]]
        y, C = op.y, op.cout
        assert op.kind == "dw" and op.ks == 3 and wg["name"].startswith("seg_dw_wgrad"), row
        g = geometry(y.N, y.H, y.W, C)
        assert wg["splits"] == g["blocks"] == query("seg_dw_wgrad_blocks", y.N, y.H, y.W, C), row
        assert wg["work"] == g["blocks"] * 9 * C, row
        cls = gpu_file.wgrad_class(g["blocks"], g["last"], g["RG"], g["gy"], g["idle"])
        assert cls in classes, ("a production launch class the GPU file does not run", row, g)
    assert n == 17, "the depthwise convs of MobileNetV2's 17 inverted residual blocks"
    assert PROGRAMS, "the fixture has depthwise rows"


# ---- the references and bounds of the GPU file, without a GPU --------------------------------------------------

F32 = torch.float32


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("case", sorted(CONV), ids=lambda v: "x".join(map(str, v)))
def test_fp32_conv_reference_inside_bounds(case, stride):
    """torch's own fp32 evaluation against the float64 reference: inside the bound the GPU file asserts."""
    op = gpu_file.conv_operands(case, stride)
    worst = 0.0
    for act in (None, 0, 1, 2):
        want, bound = gpu_file.fwd_ref(op, stride, act)
        worst = max(worst, ratio(gpu_file.fwd_ref(op, stride, act, dtype=F32)[0], want, bound))
    for acc in (0, 1):
        want, bound = gpu_file.dgrad_ref(op, stride, acc)
        worst = max(worst, ratio(gpu_file.dgrad_ref(op, stride, acc, dtype=F32)[0], want, bound))
    for act in (0, 1, 2):
        want, bound = gpu_file.fwd_ref(op, stride, None, bias_act=act)
        worst = max(worst, ratio(gpu_file.fwd_ref(op, stride, None, bias_act=act, dtype=F32)[0], want, bound))
    print(case, stride, "fp32 error / bound", worst)
    assert worst <= 0.5, "the reference alone takes at most half of the bound"


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("case", sorted(WGRAD), ids=lambda v: "x".join(map(str, v)))
def test_fp32_wgrad_reference_inside_bounds(case, lazy):
    act = WGRAD[case][5] if lazy else None
    ref, f32 = gpu_file.wgrad_ref(case, act), gpu_file.wgrad_ref(case, act, dtype=F32)
    rs = ratio(f32["slabs"], ref["slabs"], ref["slab_bound"])
    rd = ratio(f32["dw"], ref["dw"], ref["dw_bound"])
    print(case, act, "fp32 error / bound: slabs", rs, "dW", rd)
    assert rs <= 0.5 and rd <= 0.5
    if lazy and act:  # the fully clamped channels: the sum of magnitudes is 0 and so is the reference
        c = torch.arange(case[1]) % 16 == 6
        assert bool((ref["slab_bound"][:, :, c] == 0).all()) and bool((ref["slabs"][:, :, c] == 0).all())
        assert bool((ref["slab_bound"][:, :, ~c] > 0).any())


def broken(got, want, bound):
    return ratio(got, want, bound) > 1.0


def test_mutations_of_the_reference_break_the_bounds():
    """Seven ways a depthwise kernel goes wrong, each applied to the float64 reference: the comparison the GPU file
    makes must fail in at least one element."""
    f64 = torch.float64
    # 1. padding filled with act(shift) instead of 0 (lazy input)
    case, s, act = (2, 8, 6, 10), 1, 2
    op = gpu_file.conv_operands(case, s)
    want, bound = gpu_file.fwd_ref(op, s, act)
    up = F.pad(op["u"].to(f64), (1, 1, 1, 1))
    a = gpu_file.lazy_apply(up, *op["lazy"], act)[0]
    mut = F.conv2d(a, op["w"].to(f64), stride=s, padding=0, groups=case[1])
    assert mut.shape == want.shape and broken(mut, want, bound)
    assert not broken(mut[:, :, 1:-1, 1:-1], want[:, :, 1:-1, 1:-1], bound[:, :, 1:-1, 1:-1]), "only at the border"
    # 2. the right tap of the last column dropped (stride 2, even W: that tap is inside the image)
    s = 2
    op = gpu_file.conv_operands(case, s)
    want, bound = gpu_file.fwd_ref(op, s)
    w2 = op["w"].to(f64).clone()
    w2[:, :, :, :2] = 0
    mut = want.clone()
    mut[..., -1] -= gpu_file.dw_conv(op["u"].to(f64), w2, s)[..., -1]
    assert broken(mut, want, bound) and not broken(mut[..., :-1], want[..., :-1], bound[..., :-1])
    # 3. the last valid column of a ragged strip zeroed: one channel group of one row of one image
    case, s = (3, 12, 4, 7), 1
    op = gpu_file.conv_operands(case, s)
    want, bound = gpu_file.fwd_ref(op, s)
    assert want.shape[3] % TW != 0
    mut = want.clone()
    mut[1, 4:8, 2, -1] = 0
    assert broken(mut, want, bound)
    # 4. taps flipped: the forward with the data gradient's kernel, the data gradient with the forward's
    assert broken(gpu_file.dw_conv(op["u"].to(f64), op["w"].flip(2, 3), s), want, bound)
    dwant, dbound = gpu_file.dgrad_ref(op, s, 0)
    assert broken(gpu_file.dw_conv(op["dy"].to(f64), op["w"], s), dwant, dbound)
    # 5. the neighbouring image read across a border row: the batch convolved as one tall image
    N, C, H, W = case
    tall = op["u"].to(f64).permute(1, 0, 2, 3).reshape(1, C, N * H, W)
    mut = gpu_file.dw_conv(tall, op["w"], s).reshape(C, N, H, W).permute(1, 0, 2, 3)
    assert broken(mut, want, bound)
    assert not broken(mut[:, :, 1:-1], want[:, :, 1:-1], bound[:, :, 1:-1]), "only at the images' border rows"
    # 6, 7. one strip dropped from one block's slab; one strip counted twice
    wcase = (5, 96, 27, 41, 1)
    ref = gpu_file.wgrad_ref(wcase, None)
    g = ref["g"]
    a, dy = ref["op"]["u"].to(f64), ref["op"]["dy"].to(f64)
    strips, _ = gpu_file.wgrad_strips(a, dy, wcase[4], g["tww"])
    assert float((gpu_file.slabs_of(strips, g) - ref["slabs"]).abs().max()) == 0
    for b, st, sign in ((g["blocks"] - 1, g["nstrips"] - 1, -1), (0, g["spb"], +1), (17, 17 * g["spb"], -1)):
        mut = ref["slabs"].clone()
        mut[b] += sign * strips[st]
        assert broken(mut, ref["slabs"], ref["slab_bound"]), (b, st, sign)
    one = strips[g["nstrips"] - 1].t()
    assert broken(ref["dw"] - one, ref["dw"], ref["dw_bound"])
