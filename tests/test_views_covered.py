"""Which kernels the engine hands a channel-slice view, and that tests/test_gpu_views.py runs each of them on one.

For every program of tests/golden/engine_routes.json the Program is built on the CPU (build_mobilenet_unet /
build_unet only: no route picking, no library), every operand view with ld != round_up(C, 4) or off != 0 is
found, and the op is joined by index with the fixture's entry-point names.  The pair (entry point, role of the
operand that is the view) must be in view_cases.COVERAGE: an engine change that hands a view to another kernel
fails here until a GPU view test exists for it.

What a view reaches (ConvOp.forward / backward / _dgrad, PoolOp, UpsampleOp):
  inp a view  -> forward `in`, weight gradient `x`, data gradient (its bnout twin and its fallback) `out` and
                 the in-place `add` (Run.begin_write_add: add == out);
  y a view    -> forward `out`, weight gradient `dy`, data gradient `in` (a conv without BatchNorm writing a slice);
  pool input  -> seg_maxpool2_fwd `in`, seg_maxpool2_bwd `in` and `din` (the gradient buffer has the same layout);
  upsample    -> low: seg_upsample_fwd `in`, seg_upsample_bwd `din`; out: seg_upsample_fwd `out`, _bwd `dout`.
A ConvOp with BatchNorm writes its conv output to a private contiguous `y`; its `out` / `res` views are touched
only by the row-tiled BN / add kernels, whose strided-slice test is tests/test_gpu_bf16io.py::test_row_tiled_passes.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from view_cases import COVERAGE  # noqa: E402

from seg_amd import MobileNetV2UNet, UNet, deterministic_init, engine  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_routes.json")) as _fh:
    GOLDEN = json.load(_fh)
_MODELS = {}


def program(key):
    arch, shape, math = key.split()
    N, H, W = (int(v) for v in shape.split("x"))
    if arch not in _MODELS:
        _MODELS[arch] = deterministic_init({"MobileNetV2UNet": MobileNetV2UNet, "UNet": UNet}[arch](10), seed=0).train()
    build = engine.build_mobilenet_unet if arch == "MobileNetV2UNet" else engine.build_unet
    return build(_MODELS[arch], N, H, W, math), math


def is_view(a):
    return a is not None and (a.ld != engine.r4(a.C) or a.off != 0)


def _dgrad_names(d):
    out = []
    while d is not None:
        out += [d["name"]] + ([d["bnout"]] if d.get("bnout") else [])
        d = d.get("fallback")
    return out


def derive(key):
    """{(entry point, role): op index} of the program's launches that get a view."""
    prog, math = program(key)
    rows = {r["op"]: r for r in GOLDEN[key]}
    sfx = "_bf16io" if math == "bf16io" else ""
    pairs = {}

    def add(k, names, roles):
        for n in names:
            for r in roles:
                pairs.setdefault((n, r), k)

    for k, op in enumerate(prog.ops):
        if isinstance(op, engine.ConvOp):
            row = rows[k]
            assert row["conv"].endswith(f"{op.cout}"), (k, row["conv"])  # the fixture row is this op's
            dgrad = _dgrad_names(row["dgrad"])
            if is_view(op.inp):
                add(k, [row["fwd"]["name"]], ["in"])
                add(k, [row["wgrad"]["name"]], ["x"])
                add(k, dgrad, ["out", "add"])
            if is_view(op.y):
                add(k, [row["fwd"]["name"]], ["out"])
                add(k, [row["wgrad"]["name"]], ["dy"])
                add(k, dgrad, ["in"])
        elif isinstance(op, engine.PoolOp):
            if is_view(op.inp):
                add(k, ["seg_maxpool2_fwd" + sfx], ["in"])
                add(k, ["seg_maxpool2_bwd" + sfx], ["in", "din"])
            assert not is_view(op.out), "a pool writing a slice has no view test"
        elif isinstance(op, engine.UpsampleOp):
            if is_view(op.low):
                add(k, ["seg_upsample_fwd" + sfx], ["in"])
                add(k, ["seg_upsample_bwd" + sfx], ["din"])
            if is_view(op.out):
                add(k, ["seg_upsample_fwd" + sfx], ["out"])
                add(k, ["seg_upsample_bwd" + sfx], ["dout"])
        else:
            raise AssertionError(f"op {k}: {type(op).__name__} is not handled here")
    return pairs


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_every_view_has_a_gpu_test(key):
    pairs = derive(key)
    assert pairs, "every production program has a concat buffer"
    missing = sorted((p, k) for p, k in pairs.items() if p not in COVERAGE)
    assert not missing, f"(entry point, role) handed a view at op k, without a case in test_gpu_views.py: {missing}"


def test_the_skip_consumers_are_found():
    """The four convs that read a skip slice of MobileNetV2UNet's cat buffers, and UNet's pools."""
    prog, _ = program("MobileNetV2UNet 32x256x512 f32")
    got = [(k, op.cin, op.cout, op.inp.ld) for k, op in enumerate(prog.ops)
           if isinstance(op, engine.ConvOp) and is_view(op.inp)]
    assert got == [(3, 16, 96, 80), (9, 24, 144, 152), (18, 32, 192, 288), (30, 64, 384, 1344)]
    prog, _ = program("UNet 8x512x1024 f32")
    got = [(op.inp.C, op.inp.ld) for op in prog.ops if isinstance(op, engine.PoolOp)]
    assert got == [(64, 128), (128, 256), (256, 512)]
    assert ("seg_conv_igemm_bnout", "out") in derive("MobileNetV2UNet 32x256x512 f32")
    assert ("seg_maxpool2_bwd_bf16io", "din") in derive("UNet 8x512x1024 bf16io")


# The folded inference forward has no route table: its launches, by call site.
FOLDED = [
    # seg_amd/engine.py ConvOp.forward_folded, `rt.call(_FOLDED_CONV[rt.prog.math] + "_ic", rt.ptr(i), i.ld, ...
    # rt.ptr(o), o.ld, ... rt.ptr(r), r.ld ...)` (engine.py:361): input, output and residual addend as they come
    ("seg_conv_igemm_act_ic", "in"), ("seg_conv_igemm_act_ic", "out"), ("seg_conv_igemm_act_ic", "add"),
    ("seg_conv_igemm_bf16_ic", "in"), ("seg_conv_igemm_bf16_ic", "out"), ("seg_conv_igemm_bf16_ic", "add"),
    ("seg_conv_igemm_f16_ic", "in"), ("seg_conv_igemm_f16_ic", "out"), ("seg_conv_igemm_f16_ic", "add"),
    # Run.forward_folded, `call("seg_pw2_f16", self.ptr(x), x.ld, ...)` (engine.py:1372)
    ("seg_pw2_f16", "x"),
    # Run._mbconv, `call("seg_mbconv_f16", self.ptr(x), x.ld, ... self.ptr(r), r.ld, self.ptr(o), o.ld, ...)`
    # (engine.py:1395)
    ("seg_mbconv_f16", "x"), ("seg_mbconv_f16", "res"), ("seg_mbconv_f16", "out"),
    # Predictor, `call("seg_stem_pre_f16", ... rt.ptr(o), o.ld, s)` (seg_amd/infer.py:116)
    ("seg_stem_pre_f16", "out"),
]


def test_folded_inference_launches_are_covered():
    missing = [p for p in FOLDED if p not in COVERAGE]
    assert not missing, missing


def test_coverage_names_are_entry_points():
    """A typo in the table would cover nothing: every name is a bound entry point."""
    from seg_amd._lib import PROTOTYPES
    unknown = sorted({n for n, _ in COVERAGE if n not in PROTOTYPES})
    assert not unknown, unknown
