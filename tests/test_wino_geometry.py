"""CPU: the launch geometry of the Winograd kernels (csrc/wino.hip) through the library's host queries --
seg_conv_wino_geometry (the tiles, the tiles per split and the fallback decision the launches themselves use),
seg_conv_wino_fused_ok, seg_conv_wino_pick -- against include/segamd.h's comment, and what the production programs
of tests/golden/engine_routes.json ask of it: every Winograd route (forward, data gradient, weight gradient) lands on
an (entry point, variant) that tests/test_gpu_wino_matrix.py compares with float64, no weight gradient takes the
span fallback, none of their splits is empty, and their split counts stay within what the reduce test runs.

No GPU: the queries are host functions (as tests/test_wgrad_geometry.py relies on)."""
import ctypes
import importlib.util
import json
import os
import re
import sys

import pytest

from seg_amd._lib import query

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_wino_matrix as gpu_file  # noqa: E402  -- the case table only; its tests are marked gpu

_spec = importlib.util.spec_from_file_location("make_engine_routes", os.path.join(HERE, "golden",
                                                                                  "make_engine_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURE = json.load(open(os.path.join(HERE, "golden", "engine_routes.json")))
HEADER = open(os.path.join(os.path.dirname(HERE), "include", "segamd.h")).read()
DOC = HEADER[HEADER.index("Weight gradient of the same convs by Winograd"):HEADER.index("int seg_conv_wino_geometry(")]
LIMIT = (1 << 31) - 16  # the byte bound of the 31-bit buffer offsets, as the header states it
assert "2^31 - 16" in DOC


def cdiv(a, b):
    return -(-a // b)


def r4(c):
    return (c + 3) & ~3


def geometry(N, H, W, cin, cout, splits=1, ld=4):
    out = (ctypes.c_int * 6)()
    assert query("seg_conv_wino_geometry", N, H, W, cin, cout, splits, ld, ctypes.addressof(out)) == 0
    return dict(gemm=f"128x{out[0]}", wgrad=f"{out[1]}x{out[2]}", wgrad16=f"{out[3]}x{out[3]}", kchunk=out[4],
                fallback=out[5])


# ---- the header's rules, parsed (not restated) -----------------------------------------------------------------

def header_wgrad_tile(cin, cout):
    m = re.search(r"Cout >= (\d+):\s+(\d+x\d+) if Cin >= (\d+), else (\d+x\d+)\s+\*\s+(\d+) <= Cout < (\d+):\s+"
                  r"(\d+x\d+) if Cin >= (\d+), else (\d+x\d+)\s+\*\s+Cout < (\d+):\s+(\d+x\d+)", DOC)
    assert m, DOC
    v = m.groups()
    assert v[0] == v[5] and v[4] == v[9], "the three Cout ranges of the comment must meet"
    if cout >= int(v[0]):
        return v[1] if cin >= int(v[2]) else v[3]
    if cout >= int(v[4]):
        return v[6] if cin >= int(v[7]) else v[8]
    return v[10]


def header_wgrad16_tile(cin, cout):
    m = re.search(r"seg_conv_wino_wgrad16's launch: (\d+) if Cin >= (\d+) and Cout >= (\d+), else (\d+)", DOC)
    assert m, DOC
    wide, c0, c1, narrow = (int(x) for x in m.groups())
    b = wide if cin >= c0 and cout >= c1 else narrow
    return f"{b}x{b}"


def header_gemm_tile(cout):
    m = re.search(r"Cout >= (\d+) and ceil\(Cout / (\d+)\) \* (\d+) == ceil\(Cout / (\d+)\):\s+(\d+) \(8 waves\)\s+\*\s+"
                  r"otherwise Cout >= (\d+):\s+(\d+)\s+\*\s+Cout < (\d+):\s+(\d+)", DOC)
    assert m, DOC
    c0, d0, k, d1, wide, c1, mid, c2, narrow = (int(x) for x in m.groups())
    assert c1 == c2, "the Cout ranges of the comment must meet"
    if cout >= c0 and cdiv(cout, d0) * k == cdiv(cout, d1):
        return f"128x{wide}"
    return f"128x{mid if cout >= c1 else narrow}"


def header_kchunk(T, splits):
    m = re.search(r"kchunk = ceil\(T / splits\) rounded up to (\d+) tiles", DOC)
    assert m, DOC
    step = int(m.group(1))
    return cdiv(cdiv(T, splits), step) * step


def test_header_tile_rules_at_their_boundaries():
    seen = {"wgrad": set(), "wgrad16": set(), "gemm": set()}
    for cout in (32, 60, 64, 124, 128, 132, 252, 256, 260, 384, 388, 392, 512, 516, 640, 1344):
        for cin in (32, 124, 128, 132, 256):
            q = geometry(2, 8, 8, cin, cout)
            assert q["wgrad"] == header_wgrad_tile(cin, cout), (cin, cout, q)
            assert q["wgrad16"] == header_wgrad16_tile(cin, cout), (cin, cout, q)
            assert q["gemm"] == header_gemm_tile(cout), (cin, cout, q)
            for k in seen:
                seen[k].add(q[k])
    assert seen["wgrad"] == {"128x128", "128x64", "64x128", "64x64", "32x128"}
    assert seen["wgrad16"] == {"64x64", "32x32"} and seen["gemm"] == {"128x64", "128x128", "128x256"}
    pairs, _ = gpu_file.covered()
    assert {v for e, v in pairs if e == "seg_conv_wino_wgrad"} == seen["wgrad"], "the GPU file claims every tile"
    assert {v for e, v in pairs if e == "seg_conv_wino_wgrad16"} == seen["wgrad16"]
    assert {v for e, v in pairs if e == "seg_conv_wino"} == seen["gemm"]
    assert ("seg_conv_wino_fused", gpu_file.FUSED_TILE) in pairs


def test_gpu_file_cases_land_where_they_claim():
    g = gpu_file.GEO
    assert (g.N, g.H, g.W, g.T) == (3, 14, 14, 147)
    for (cin, cout), tile in gpu_file.CASES["conv"].items():
        assert geometry(g.N, g.H, g.W, cin, cout)["gemm"] == tile == header_gemm_tile(cout)
    for (cin, cout, creal), tiles in gpu_file.CASES["wgrad"].items():
        q = geometry(g.N, g.H, g.W, cin, cout)
        assert (q["wgrad"], q["wgrad16"]) == tiles == (header_wgrad_tile(cin, cout), header_wgrad16_tile(cin, cout))
        assert r4(creal) == cin
    assert gpu_file.SPLITS == (1, 3, 7, 40)
    ks = [geometry(g.N, g.H, g.W, 72, 72, s)["kchunk"] for s in gpu_file.SPLITS]
    assert ks == [160, 64, 32, 16] and [cdiv(g.T, k) for k in ks] == [1, 3, 5, 10]
    # the fold runs of seg_conv_wino_wgrad_reduce (above 16 splits: runs of L = ceil(splits / 16) slabs)
    runs = [(1 if s <= 16 else cdiv(s, 16)) for s in gpu_file.REDUCE_SPLITS]
    assert runs == [1, 1, 2, 3, 11, 32, 64]
    assert 169 - (cdiv(169, 11) - 1) * 11 == 4, "169 splits: the last run holds 4 slabs"


SWEEP_T = ((1, 2, 2), (5, 2, 2), (3, 14, 14), (2, 30, 34), (8, 64, 128), (32, 128, 256), (8, 512, 1024))
SWEEP_SPLITS = (1, 2, 7, 40, 169, 512, 1023, 1024)


def test_kchunk_sweep():
    for N, H, W in SWEEP_T:
        T = N * (H // 2) * (W // 2)
        for splits in SWEEP_SPLITS:
            for cin, cout in ((32, 32), (72, 136), (256, 256)):
                k = geometry(N, H, W, cin, cout, splits)["kchunk"]
                assert k == header_kchunk(T, splits), (N, H, W, splits)
                assert k > 0 and splits * k >= T, "every tile belongs to a split"


def test_refused_arguments():
    out = (ctypes.c_int * 6)(*([-7] * 6))
    for args in ((3, 13, 14, 8, 8, 1, 8), (3, 14, 13, 8, 8, 1, 8), (3, 14, 14, 6, 8, 1, 8), (3, 14, 14, 8, 6, 1, 8),
                 (3, 14, 14, 8, 8, 0, 8), (3, 14, 14, 8, 8, 1, 6), (0, 14, 14, 8, 8, 1, 8), (-1, 14, 14, 8, 8, 1, 8),
                 (3, 14, 14, 0, 8, 1, 8), (1 << 20, 128, 128, 8, 8, 1, 8)):
        assert query("seg_conv_wino_geometry", *args, ctypes.addressof(out)) == 1, args  # hipErrorInvalidValue
        assert tuple(out) == (-7,) * 6, "a refused query writes nothing"
    assert query("seg_conv_wino_geometry", 3, 14, 14, 8, 8, 1, 8, None) == 1
    # the launches refuse the same shapes on the host (nothing is launched; no GPU is needed)
    for N, H, W, cin, cout in ((3, 13, 14, 8, 8), (3, 14, 13, 8, 8), (3, 14, 14, 6, 8), (3, 14, 14, 8, 6)):
        assert query("seg_conv_wino", None, 8, N, H, W, cin, None, 8, None, None, 8, cout, None, 0, None, None,
                     None) == 1
        assert query("seg_conv_wino_fused", None, 8, N, H, W, cin, None, 8, None, None, 8, cout, None, 0, None,
                     None) == 1
        for name in ("seg_conv_wino_wgrad", "seg_conv_wino_wgrad16"):
            assert query(name, None, 8, None, 8, N, H, W, cin, cout, None, 1, None) == 1
    for name in ("seg_conv_wino_wgrad", "seg_conv_wino_wgrad16"):
        assert query(name, None, 8, None, 8, 3, 14, 14, 8, 8, None, 0, None) == 1   # splits < 1
        assert query(name, None, 6, None, 8, 3, 14, 14, 8, 8, None, 1, None) == 1   # lddy % 4
        assert query(name, None, 8, None, 6, 3, 14, 14, 8, 8, None, 1, None) == 1   # ldx % 4


def test_pick_refuses_what_the_kernels_cannot_run():
    assert query("seg_conv_wino_pick", 8, 64, 128, 256, 256) == 1
    assert query("seg_conv_wino_pick", 8, 64, 128, 152, 64) == 2
    for args in ((8, 63, 128, 256, 256), (8, 64, 127, 256, 256), (8, 64, 128, 254, 256), (8, 64, 128, 256, 254),
                 (8, 63, 128, 152, 64), (8, 64, 128, 150, 64), (8, 64, 128, 152, 66)):
        assert query("seg_conv_wino_pick", *args) == 0, args


def test_31_bit_rules_flip_where_the_header_says():
    """seg_conv_wino_fused_ok: min(N, 128 / tiles per image + 2) * H * W * ldin * 4 < 2^31 - 16; the fallback flag of
    seg_conv_wino_wgrad16: (2 * (ceil(kchunk / (W/2)) + 1) + 2) * W * ld * 4 >= 2^31 - 16.  Each probed at the
    largest ld (a multiple of 4) that fits and the next one."""
    assert "min(N, 128 / ((H/2) * (W/2)) + 2) * H * W * ldin * 4 < 2^31 - 16" in DOC
    assert "(2 * (ceil(kchunk / (W/2)) + 1) + 2) * W * max(ldx, lddy) * 4 >= 2^31 - 16" in DOC
    for N, H, W in ((3, 14, 14), (5, 2, 2), (1, 2, 2), (32, 128, 256), (8, 512, 1024), (2, 64, 128)):
        unit = min(N, 128 // ((H // 2) * (W // 2)) + 2) * H * W * 4
        ld = (LIMIT - 1) // unit // 4 * 4  # the largest multiple of 4 with unit * ld < LIMIT
        assert unit * ld < LIMIT <= unit * (ld + 4)
        assert query("seg_conv_wino_fused_ok", N, H, W, ld) == 1, (N, H, W, ld)
        assert query("seg_conv_wino_fused_ok", N, H, W, ld + 4) == 0, (N, H, W, ld)
        for splits in (1, 7, 512):
            k = geometry(N, H, W, 64, 64, splits)["kchunk"]
            unit = (2 * (cdiv(k, W // 2) + 1) + 2) * W * 4
            ld = (LIMIT - 1) // unit // 4 * 4
            assert unit * ld < LIMIT <= unit * (ld + 4)
            assert geometry(N, H, W, 64, 64, splits, ld)["fallback"] == 0, (N, H, W, splits, ld)
            assert geometry(N, H, W, 64, 64, splits, ld + 4)["fallback"] == 1, (N, H, W, splits, ld)


# ---- the production programs ----------------------------------------------------------------------------------

PROGRAMS = [(arch, N, H, W) for arch, N, H, W, maths in gen.PROGRAMS if "f32" in maths]


@pytest.mark.parametrize("arch,N,H,W", PROGRAMS, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" for c in PROGRAMS])
def test_production_routes(arch, N, H, W):
    prog = gen.build(arch, N, H, W, "f32")
    pairs, reduce_splits = gpu_file.covered()
    used, n_w = set(), 0
    for row in FIXTURE[f"{arch} {N}x{H}x{W} f32"]:
        op = prog.ops[row["op"]]
        y = op.y
        for d, key in enumerate(("fwd", "dgrad")):
            r = row[key]
            if not r or not r["name"].startswith("seg_conv_wino"):
                continue
            K, C = (r4(op.cout), op.cin) if d else (op.cin_pad, op.cout)
            assert r["ldk"] == K and query("seg_conv_wino_pick", y.N, y.H, y.W, K, C) in (1, 2), row
            q = geometry(y.N, y.H, y.W, K, C)
            if r["name"] == "seg_conv_wino":
                assert r["work"] == 16 * (y.M // 4) * C, row
                used.add(("seg_conv_wino", q["gemm"]))
            else:
                assert r["name"] == "seg_conv_wino_fused" and r["work"] == 0, row
                src_ld = (r4(op.cout) if op.bn is not None else op.out.ld) if d else op.inp.ld
                assert query("seg_conv_wino_fused_ok", y.N, y.H, y.W, src_ld) == 1, row
                used.add(("seg_conv_wino_fused", gpu_file.FUSED_TILE))
        wg = row["wgrad"]
        if wg and wg["name"].startswith("seg_conv_wino"):
            n_w += 1
            K, cout, splits = op.cin_pad, op.cout, wg["splits"]
            assert op.ks == 3 and op.stride == 1 and K == r4(op.cin), row
            assert splits == query(wg["name"] + "_splits", y.N, y.H, y.W, K, cout), row
            assert wg["work"] == splits * 16 * cout * K, row
            ld = max(op.inp.ld, r4(cout) if op.bn is not None else op.out.ld)  # ldx, lddy: ConvOp.backward
            q = geometry(y.N, y.H, y.W, K, cout, splits, ld)
            T = y.N * (y.H // 2) * (y.W // 2)
            assert splits * q["kchunk"] >= T, row
            assert (splits - 1) * q["kchunk"] < T, ("production launches a split without tiles", row)
            assert splits <= max(reduce_splits), ("a split count beyond what the reduce test runs", row)
            if wg["name"] == "seg_conv_wino_wgrad16":
                assert q["fallback"] == 0, ("a production weight gradient takes the span fallback", row)
                used.add(("seg_conv_wino_wgrad16", q["wgrad16"]))
            else:
                used.add(("seg_conv_wino_wgrad", q["wgrad"]))
    assert n_w and any(e == "seg_conv_wino" for e, _ in used), "every f32 program has Winograd routes"
    assert used <= pairs, used - pairs
