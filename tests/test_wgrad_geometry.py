"""CPU: the split geometry of the implicit-GEMM weight gradient (csrc/wgrad.hip) through the library's host
queries -- seg_conv_wgrad_geometry (the tile and the pixels per split the launch itself uses), seg_conv_wgrad_splits
and seg_conv_wgrad_splits_bf16 -- and what the production programs of tests/golden/engine_routes.json ask of it:
their split counts, workspace sizes, that none of their splits is empty, and that every (tile, math, xf) they launch
is among those tests/test_gpu_wgrad_matrix.py compares with float64.

No GPU: the queries are host functions (as tests/test_igemm_tiles.py relies on)."""
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
import test_gpu_wgrad_matrix as gpu_file  # noqa: E402  -- the case table only; its tests are marked gpu

_spec = importlib.util.spec_from_file_location("make_engine_routes", os.path.join(HERE, "golden",
                                                                                  "make_engine_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURE = json.load(open(os.path.join(HERE, "golden", "engine_routes.json")))
MATH = {"seg_conv_wgrad": "f32", "seg_conv_wgrad_bf16": "bf16", "seg_conv_wgrad_bf16io": "bf16io"}


def cdiv(a, b):
    return -(-a // b)


def r4(c):
    return (c + 3) & ~3


def geometry(M, cout, cin, ks, splits, bf16):
    out = (ctypes.c_int * 3)()
    assert query("seg_conv_wgrad_geometry", M, cout, cin, ks, splits, bf16, ctypes.addressof(out)) == 0
    return (out[0], out[1]), out[2]


def header_rule(cout, nw):
    """The tile rule as include/segamd.h's comment on seg_conv_wgrad states it (parsed, not restated)."""
    text = open(os.path.join(os.path.dirname(HERE), "include", "segamd.h")).read()
    block = text[text.index("Tile (rows of Cout x columns of Nw"):text.index("int seg_conv_wgrad_splits(")]
    m = re.search(r"Cout >= (\d+):\s+(\d+)x(\d+) if Nw >= (\d+), else (\d+)x(\d+)\s+\*\s+(\d+) <= Cout < (\d+):\s+"
                  r"(\d+)x(\d+) if Nw >= (\d+), else (\d+)x(\d+)\s+\*\s+Cout < (\d+):\s+(\d+)x(\d+)", block)
    assert m, block
    v = [int(x) for x in m.groups()]
    assert v[0] == v[7] and v[6] == v[13], "the three Cout ranges of the comment must meet"
    if cout >= v[0]:
        return (v[1], v[2]) if nw >= v[3] else (v[4], v[5])
    if cout >= v[6]:
        return (v[8], v[9]) if nw >= v[10] else (v[11], v[12])
    return v[14], v[15]


def test_header_tile_rule_at_its_boundaries():
    seen = set()
    for cout in (63, 64, 127, 128):
        for cin in (124, 128):  # ks 1: Nw 124 / 128; Nw 127 is no multiple of 4, so 124 stands below the boundary
            tile, _ = geometry(1000, cout, cin, 1, 1, 0)
            assert tile == header_rule(cout, cin), (cout, cin)
            assert header_rule(cout, 127) == header_rule(cout, 124)
            seen.add(tile)
        assert geometry(1000, cout, 12, 3, 1, 1)[0] == header_rule(cout, 108)
        assert geometry(1000, cout, 16, 3, 1, 1)[0] == header_rule(cout, 144)
    assert seen == {(32, 128), (64, 64), (64, 128), (128, 32), (128, 128)}
    assert seen == {CASE[0] for CASE in gpu_file.CASES.values()}, "the GPU file claims every tile, and no other"


def test_refused_arguments():
    out = (ctypes.c_int * 3)(-7, -7, -7)
    for args in ((234, 64, 6, 1, 1, 0), (234, 64, 8, 2, 1, 0), (234, 64, 8, 5, 1, 1), (234, 64, 8, 1, 0, 0),
                 (234, 64, 8, 3, -1, 1), (0, 64, 8, 1, 1, 0), (234, 0, 8, 1, 1, 0), (1 << 31, 64, 8, 1, 1, 0)):
        assert query("seg_conv_wgrad_geometry", *args, ctypes.addressof(out)) == 1, args  # hipErrorInvalidValue
        assert tuple(out) == (-7, -7, -7), "a refused query writes nothing"
    assert query("seg_conv_wgrad_geometry", 234, 64, 8, 1, 1, 0, None) == 1


SWEEP_M = (1, 70, 234, 255, 256, 257, 4097, 8 * 300 * 500, 32 * 256 * 512)
SWEEP_SPLITS = (1, 2, 7, 40, 1023, 1024)


@pytest.mark.parametrize("bf16", (0, 1))
def test_kchunk_sweep(bf16):
    bk = 32 if bf16 else 16  # pixels per K step: SEG_WGRAD_BK / SEG_WGRAD_BK_BF16 (csrc/wgrad.hip)
    for M in SWEEP_M:
        for splits in SWEEP_SPLITS:
            for cout, cin, ks in ((32, 4, 3), (144, 24, 1), (64, 192, 1)):
                _, kchunk = geometry(M, cout, cin, ks, splits, bf16)
                assert kchunk % bk == 0 and kchunk > 0
                assert splits * kchunk >= M, "every pixel belongs to a split"
                assert kchunk - cdiv(M, splits) < bk, "rounded up by less than one K step"


def test_forced_splits_leave_empty_trailing_splits():
    """The rounding to whole K steps leaves trailing splits without pixels: the case the GPU test covers (an empty
    split writes an all-zero slab)."""
    M = 8 * 300 * 500
    for bf16, want in ((0, 1184), (1, 1184)):
        _, kchunk = geometry(M, 32, 4, 3, 1024, bf16)
        assert kchunk == want
        assert cdiv(M, kchunk) == 1014, "the last 10 of 1024 splits start past M"
        assert (1024 - 1) * kchunk >= M
    # the GPU file's own shapes: M = 234 (stride 1) and 70 (stride 2)
    assert gpu_file.SPLITS == (1, 3, 7, 40)
    filled = {(M, bf16, s): cdiv(M, geometry(M, 64, 16, 1, s, bf16)[1]) for M in (234, 70) for bf16 in (0, 1)
              for s in gpu_file.SPLITS}
    assert [geometry(234, 64, 16, 1, s, 0)[1] for s in gpu_file.SPLITS] == [240, 80, 48, 16]
    assert [geometry(234, 64, 16, 1, s, 1)[1] for s in gpu_file.SPLITS] == [256, 96, 64, 32]
    assert [filled[234, 0, s] for s in gpu_file.SPLITS] == [1, 3, 5, 15]
    assert [filled[234, 1, s] for s in gpu_file.SPLITS] == [1, 3, 4, 8]
    assert [filled[70, 0, s] for s in gpu_file.SPLITS] == [1, 3, 5, 5]
    assert [filled[70, 1, s] for s in gpu_file.SPLITS] == [1, 3, 3, 3]


def test_split_count_queries():
    for name in ("seg_conv_wgrad_splits", "seg_conv_wgrad_splits_bf16"):
        for M in SWEEP_M:
            for cout, cin, ks in ((32, 4, 3), (10, 16, 1), (144, 24, 1), (64, 192, 1), (1280, 320, 1), (256, 1344, 3)):
                s = query(name, M, cout, cin, ks)
                assert 1 <= s <= 1024, (name, M, cout, cin, ks, s)
                assert s <= max(1, M // 256), "at least 256 pixels per split"


# ---- the production programs ----------------------------------------------------------------------------------

PROGRAMS = [(arch, N, H, W, math) for arch, N, H, W, maths in gen.PROGRAMS for math in maths]


def wgrad_routes(arch, N, H, W, math):
    """(fixture row, op) of every seg_conv_wgrad* route of one program (seg_conv_wgrad2_bf16io is another kernel)."""
    prog = gen.build(arch, N, H, W, math)
    out = []
    for row in FIXTURE[f"{arch} {N}x{H}x{W} {math}"]:
        wg = row["wgrad"]
        if wg and wg["name"].startswith("seg_conv_wgrad") and wg["family"] != "wgrad2":
            assert wg["family"] == "igemm"
            out.append((row, prog.ops[row["op"]]))
    return out


@pytest.mark.parametrize("arch,N,H,W,math", PROGRAMS, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}" for c in PROGRAMS])
def test_production_routes(arch, N, H, W, math):
    routes = wgrad_routes(arch, N, H, W, math)
    assert routes, "every program has implicit-GEMM weight gradients"
    used = set()
    for row, op in routes:
        wg = row["wgrad"]
        name, xf = (wg["name"][:-3], True) if wg["name"].endswith("_xf") else (wg["name"], False)
        assert MATH[name] == math, row
        assert xf == (op.xform is not None)
        bf16 = int(math != "f32")
        M, cout, cin, ks = op.y.M, op.cout, op.cin_pad, op.ks
        assert cin == r4(op.cin) and row["conv"] == f"{ks}x{ks}s{op.stride} {op.cin}->{cout}"
        splits = wg["splits"]
        assert splits == query("seg_conv_wgrad_splits_bf16" if bf16 else "seg_conv_wgrad_splits", M, cout, cin, ks), row
        assert wg["work"] == splits * cout * ks * ks * cin, row
        tile, kchunk = geometry(M, cout, cin, ks, splits, bf16)
        assert splits * kchunk >= M, row
        assert (splits - 1) * kchunk < M, ("production launches a split without pixels", row)
        used.add((tile, math, xf, ks, op.stride))
    assert {u[:3] for u in used} <= gpu_file.covered(), used
    # and with the kernel size and stride, which select the instantiation with them
    assert used <= gpu_file.covered(kernel=True), used - gpu_file.covered(kernel=True)
