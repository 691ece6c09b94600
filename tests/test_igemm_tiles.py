"""CPU: the implicit GEMM's tile table (csrc/igemm_impl.h kTiles, documented in include/segamd.h) through the
library's host functions -- the forcing hook, the row / output tile geometry of every entry, which entries take the
BN-backward-partials epilogue -- and which entries the production programs of tests/golden/engine_routes.json
launch: every one of them must be among the tiles tests/test_gpu_igemm_tiles.py runs against float64.

No GPU: seg_igemm_force_tile and the seg_conv_igemm_* queries are host functions (as tests/test_engine_routes.py
relies on)."""
import collections
import ctypes
import importlib.util
import os
import re

import pytest

from seg_amd import engine
from seg_amd._lib import query

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_engine_routes", os.path.join(HERE, "golden",
                                                                                  "make_engine_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GPU_TEST_TILES = range(15)  # tests/test_gpu_igemm_tiles.py's `tile` parameter


def header_tiles():
    """[(BM, BN, waves)] by index, from the table in include/segamd.h's comment on seg_igemm_force_tile."""
    text = open(os.path.join(os.path.dirname(HERE), "include", "segamd.h")).read()
    block = text[text.index("The implicit GEMM's tile table"):text.index("int seg_igemm_force_tile")]
    rows = {int(i): (int(bm), int(bn), int(w)) for i, bm, bn, w in re.findall(r"\b(\d+)\s+(\d+)x(\d+)\s+([48])\b", block)}
    assert sorted(rows) == list(range(len(rows)))
    return [rows[i] for i in range(len(rows))]


TILES = header_tiles()


@pytest.fixture(autouse=True)
def cost_model_again():
    try:
        yield
    finally:
        engine.force_tiles(igemm=-1)


def cdiv(a, b):
    return -(-a // b)


def test_the_table_has_fifteen_entries_and_the_gpu_test_runs_them_all():
    assert len(TILES) == 15 and list(GPU_TEST_TILES) == list(range(len(TILES)))
    assert all(w == 4 for _, _, w in TILES[:8]) and all(w == 8 for _, _, w in TILES[8:])


def test_force_tile_range():
    for t in (-1, 0, 7, 8, 14):
        assert query("seg_igemm_force_tile", t) == 0
        assert query("seg_conv_igemm_tile", 1000, 64) == t or t == -1
    assert query("seg_igemm_force_tile", 3) == 0
    for t in (15, -2, 100):
        assert query("seg_igemm_force_tile", t) != 0
        assert query("seg_conv_igemm_tile", 1000, 64) == 3, "a refused value must leave the hook as it was"
    assert query("seg_igemm_force_tile", -1) == 0
    assert 0 <= query("seg_conv_igemm_tile", 1000, 64) <= 7  # the cost model picks among the 4-wave tiles


@pytest.mark.parametrize("t", range(15))
def test_forced_tile_geometry(t):
    """Row tiles (kernel statistics rows), output tiles (split-K counters) and the BN-backward epilogue's tiles
    follow the documented BM x BN of the forced entry."""
    bm, bn, _ = TILES[t]
    engine.force_tiles(igemm=t)
    rows = ctypes.c_int(0)
    assert query("seg_conv_igemm_row_tiles", 1000, 64, ctypes.addressof(rows)) == cdiv(1000, bm)
    assert rows.value == bm
    assert query("seg_conv_igemm_row_tiles", 1000, 64, None) == cdiv(1000, bm)
    for M, C in ((1000, 64), (300, 266), (1, 1), (65536, 1280)):
        assert query("seg_conv_igemm_tile", M, C) == t
        assert query("seg_conv_igemm_tiles", M, C) == cdiv(M, bm) * cdiv(C, bn), (M, C)
    for bf16, vo in ((0, 4), (1, 8)):  # one 16-byte column vector per lane: 64 % (BN / vo) == 0
        want = int(bn % vo == 0 and 64 % (bn // vo) == 0)
        assert query("seg_conv_igemm_bnout_ok", 300, 266, bf16) == want
        assert want == int(t not in (4, 5))


def igemm_launches(prog):
    """(M, Cout) of every generic implicit-GEMM launch of a program: forwards, data gradients and the implicit-GEMM
    fallbacks of data gradients routed elsewhere (engine._pick_conv: a forward writes y [M][cout], a stride-1 data
    gradient writes dx [M][cin])."""
    out = []
    for op in prog.ops:
        if not isinstance(op, engine.ConvOp):
            continue
        if op.route_f is not None and op.route_f.family == "igemm":
            out.append(("fwd", op.y.M, op.cout))
        r = op.route_d
        while r is not None:
            if r.family == "igemm":
                out.append(("dgrad", op.inp.M, op.cin))
            r = r.fallback
    return out


# the tiles each production program's generic implicit-GEMM launches get from the cost model
PRODUCTION = {
    "MobileNetV2UNet 32x256x512 f32": {1, 4, 5, 7},
    "MobileNetV2UNet 32x256x512 bf16": {0, 1, 2, 4, 5, 7},
    "MobileNetV2UNet 32x256x512 bf16io": {0, 1, 4, 5, 7},
    "UNet 8x512x1024 f32": {2, 7},
    "UNet 8x512x1024 bf16io": {0, 2, 7},
}
CASES = [(arch, N, H, W, math) for arch, N, H, W, maths in gen.PROGRAMS for math in maths]


@pytest.mark.parametrize("arch,N,H,W,math", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}" for c in CASES])
def test_production_tiles_are_tested_tiles(arch, N, H, W, math):
    key = f"{arch} {N}x{H}x{W} {math}"
    launches = igemm_launches(gen.build(arch, N, H, W, math))
    assert launches, "every program has implicit-GEMM launches"
    used = collections.Counter(query("seg_conv_igemm_tile", M, C) for _, M, C in launches)
    assert set(used) <= set(GPU_TEST_TILES), used
    if key in PRODUCTION:
        assert set(used) == PRODUCTION[key], dict(used)


def test_batch1_plan_tiles_are_tested_tiles():
    """seg_conv_igemm_plan_b1 (the folded inference forward) names tiles 3 and 12 besides the cost model's."""
    plan = (ctypes.c_int * 3)()
    seen = set()
    for H, W, cin, cout, ks in ((8, 16, 1344, 256, 3), (16, 32, 288, 128, 3), (32, 64, 152, 64, 3),
                                (64, 128, 32, 32, 3), (4, 8, 320, 1280, 1), (128, 256, 16, 96, 1)):
        assert query("seg_conv_igemm_plan_b1", H * W, cout, cin, ks, ctypes.addressof(plan)) == 0
        seen.add(plan[1] if plan[1] >= 0 else query("seg_conv_igemm_tile", H * W, cout))
    assert {3, 12} <= seen <= set(GPU_TEST_TILES), seen
