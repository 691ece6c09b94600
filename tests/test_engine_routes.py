"""Kernel routing (seg_amd.engine.pick_routes) on the CPU: which entry point runs each conv's forward, data gradient
and weight gradient, with which statistics tiling, workspace and packed weight.  The picker is a pure function of
shapes, conv math, engine switches and the library's host-side queries, so this needs the built library (as
tests/test_abi.py::test_host_side_queries does) and no GPU.

Fixture tests/golden/engine_routes.json: the routes of bench.py's configurations and of the GPU suite's small shape,
derived from the engine before it had routes (tests/golden/make_engine_routes.py reproduces it byte for byte).
"""
import collections
import importlib.util
import json
import os

import pytest

from seg_amd import engine

_spec = importlib.util.spec_from_file_location(
    "make_engine_routes", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_engine_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = [(arch, N, H, W, math) for arch, N, H, W, maths in gen.PROGRAMS for math in maths]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "engine_routes.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("arch,N,H,W,math", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}" for c in CASES])
def test_route_table(golden, arch, N, H, W, math):
    """Per op: the (forward, data gradient, weight gradient) entry points, timer kinds, statistics geometry, workspace
    floats, split counts and ldk equal the committed table."""
    got = gen.table(gen.build(arch, N, H, W, math))
    want = golden[f"{arch} {N}x{H}x{W} {math}"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g["op"], g["conv"])


def _counts(rows):
    """Routes per family and direction; a forward implicit GEMM applying a lazy producer BN on load counts as xf."""
    fwd = collections.Counter("xf" if r["fwd"]["family"] == "igemm" and "_xf" in r["fwd"]["name"]
                              else r["fwd"]["family"] for r in rows)
    dgrad = collections.Counter("none" if r["dgrad"] is None else r["dgrad"]["family"] for r in rows)
    return dict(fwd), dict(dgrad), dict(collections.Counter(r["wgrad"]["family"] for r in rows))


# route counts of the engine before it had routes (the fixture must agree with them)
COUNTS = {
    "MobileNetV2UNet 32x256x512 f32": (
        {"dw": 17, "xf": 16, "igemm": 15, "pw": 6, "wino": 4, "halo": 3, "wino_fused": 1},
        {"igemm": 33, "dw": 17, "pw": 4, "wino": 3, "wino_fused": 2, "halo": 2, "none": 1},
        {"igemm": 37, "dw": 17, "wino16": 8}),
    "MobileNetV2UNet 32x256x512 bf16io": (
        {"dw": 17, "xf": 17, "igemm": 15, "pw": 5, "igemm2": 4, "halo": 4},
        {"igemm": 34, "dw": 17, "pw": 4, "igemm2": 4, "halo": 2, "none": 1},
        {"igemm": 41, "dw": 17, "wgrad2": 4}),
    "UNet 8x512x1024 f32": (
        {"wino": 7, "halo": 5, "igemm": 2, "wino_fused": 1, "pw": 1},
        {"wino": 7, "halo": 4, "wino_fused": 2, "pw": 1, "igemm": 1, "none": 1},
        {"wino16": 13, "igemm": 3}),
    "UNet 8x512x1024 bf16io": (
        {"igemm2": 8, "halo": 5, "igemm": 2, "xf": 1},
        {"igemm2": 9, "halo": 4, "pw": 1, "igemm": 1, "none": 1},
        {"igemm": 11, "wgrad2": 5}),
}


@pytest.mark.parametrize("key", sorted(COUNTS))
def test_fixture_route_counts(golden, key):
    assert _counts(golden[key]) == COUNTS[key]


def _routes(prog):
    """Every Route of a program, fallbacks included."""
    out = []
    for op in prog.ops:
        if isinstance(op, engine.ConvOp):
            for r in (op.route_f, op.route_d, op.route_w):
                while r is not None:
                    out.append(r)
                    r = r.fallback
    return out


# (switch, program, what no route may be with the switch off -- and some route is with it on)
SWITCHES = [
    ("WINOGRAD", ("UNet", 8, 512, 1024, "f32"), lambda r: r.name.startswith("seg_conv_wino")),
    ("WINOGRAD", ("MobileNetV2UNet", 32, 256, 512, "f32"), lambda r: r.name.startswith("seg_conv_wino")),
    ("HALO_BF16", ("UNet", 2, 64, 128, "bf16io"), lambda r: r.family == "halo"),
    ("WGRAD2", ("UNet", 2, 64, 128, "bf16io"), lambda r: r.family == "wgrad2"),
    ("IGEMM2", ("UNet", 2, 64, 128, "bf16io"), lambda r: r.family == "igemm2"),
    ("IGEMM2", ("UNet", 8, 512, 1024, "bf16io"), lambda r: r.family == "igemm2"),
    ("PW", ("MobileNetV2UNet", 32, 256, 512, "f32"), lambda r: r.family == "pw"),
    ("PW", ("MobileNetV2UNet", 32, 256, 512, "bf16io"), lambda r: r.family == "pw"),
    # bf16 packed weights: the _w16 entry points, and the kernels that only take them
    ("W16", ("MobileNetV2UNet", 32, 256, 512, "bf16io"),
     lambda r: "_w16" in r.name or (r.mode or 0) & 16 or r.family in ("pw", "igemm2")),
]


@pytest.mark.parametrize("switch,case,hit", SWITCHES, ids=[f"{s[0]}-{s[1][0]}-{s[1][1]}-{s[1][4]}" for s in SWITCHES])
def test_switch_off_removes_its_family(monkeypatch, switch, case, hit):
    assert any(hit(r) for r in _routes(gen.build(*case))), "the switch's family does not occur in this program"
    monkeypatch.setattr(engine, switch, False)
    bad = [r for r in _routes(gen.build(*case)) if hit(r)]
    assert not bad, bad[:3]


def test_engine_routes_wide_convs_to_igemm2(monkeypatch):
    """UNet(10) bf16io at 8x512x1024 (configs[4]): past the 65k-row cap, the 3x3 convs whose GEMM N is a multiple
    of 128 take igemm2 (SEG_IGEMM2_WIDE), the others keep the implicit GEMM / LDS halo; off: none past the cap."""
    for wide in (True, False):
        monkeypatch.setattr(engine, "IGEMM2_WIDE", wide)
        prog = gen.build("UNet", 8, 512, 1024, "bf16io")
        big = [op for op in prog.ops if isinstance(op, engine.ConvOp) and op.ks == 3 and op.y.M > 65536]
        assert big
        ig2_f = lambda op: op.route_f.family == "igemm2"  # noqa: E731
        ig2_d = lambda op: op.route_d is not None and op.route_d.family == "igemm2"  # noqa: E731
        for op in big:
            if wide and op.cout % 128 == 0 and op.cin_pad == op.cin and not op.route_f.family == "halo":
                assert ig2_f(op), (op.cin, op.cout, op.y.M)
            if op.cout % 128 or not wide:
                assert not ig2_f(op), (op.cin, op.cout, op.y.M)
            if not op.first and (op.cin % 128 or not wide):
                assert not ig2_d(op), (op.cin, op.cout, op.y.M)
        if wide:
            assert sum(ig2_f(op) for op in big) >= 4 and sum(ig2_d(op) for op in big) >= 4


class _Walk:
    """What Program.pack needs of a run: a stream handle and somewhere to put its launch."""
    stream = 0

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append(name)


def test_forced_tile_repicks_routes():
    """force_tiles drops every program's routes: the next walk (Program.pack) picks them again with the forced tile's
    statistics geometry, and -1 (the cost model) restores the original table.  Without it a walk keeps its routes."""
    prog = gen.build("UNet", 2, 64, 128, "f32")
    rt = _Walk()
    try:
        prog.pack(rt)
        first = [op.route_f for op in prog.ops if isinstance(op, engine.ConvOp)]
        table0 = gen.table(prog)
        prog.pack(rt)
        assert all(a is b for a, b in zip(first, (op.route_f for op in prog.ops if isinstance(op, engine.ConvOp))))
        assert rt.calls == ["seg_pack_batch"] * 2
        forced = []
        for tile in range(15):  # seg_igemm_force_tile: configurations 0..14
            engine.force_tiles(igemm=tile)
            prog.pack(rt)
            forced.append(gen.table(prog))
        # the tile heights differ, so no single geometry can hold for all the forced tiles
        assert any(t != table0 for t in forced)
        assert any(a is not b for a, b in zip(first, (op.route_f for op in prog.ops if isinstance(op, engine.ConvOp))))
        engine.force_tiles(igemm=-1)
        prog.pack(rt)
        assert gen.table(prog) == table0
    finally:
        engine.force_tiles(igemm=-1)
