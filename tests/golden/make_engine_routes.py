"""Generate tests/golden/engine_routes.json: the kernel route of every conv (forward, data gradient, weight
gradient) of the benchmark's programs and of the GPU suite's small shape, as seg_amd.engine.pick_routes chooses them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_engine_routes.py

Needs the built library (its host-side queries) and no GPU.  The committed table was first derived from the engine
before it had routes (per-op flags mapped to entry points by the order of its launch chains); this generator
reproduces that file byte for byte.  tests/test_engine_routes.py imports PROGRAMS, build and table from here.
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "team02-objectdetection_amd"))

from seg_amd import MobileNetV2UNet, UNet, deterministic_init, engine  # noqa: E402

# bench.py's configurations and the GPU suite's small shape: (model, N, H, W, conv maths)
PROGRAMS = (("MobileNetV2UNet", 32, 256, 512, ("f32", "bf16", "bf16io")),
            ("UNet", 8, 512, 1024, ("f32", "bf16io")),
            ("UNet", 2, 64, 128, ("f32", "bf16io")))
_MODELS = {}


def build(arch, N, H, W, math):
    """The program of a CPU model (routes need no device) with its routes picked."""
    if arch not in _MODELS:
        _MODELS[arch] = deterministic_init({"MobileNetV2UNet": MobileNetV2UNet, "UNet": UNet}[arch](10), seed=0).train()
    prog = engine.build_program(_MODELS[arch], N, H, W, math)
    engine.pick_routes(prog)
    return prog


def _row(r, keys):
    return None if r is None else {k: _row(r.fallback, keys) if k == "fallback" else
                                   list(r.tiles) if k == "tiles" and r.tiles else getattr(r, k) for k in keys}


def table(prog):
    """One row per ConvOp, in program order."""
    out = []
    for n, op in enumerate(prog.ops):
        if isinstance(op, engine.ConvOp):
            dw = op.kind == "dw"
            conv = f"{op.ks}x{op.ks}s{op.stride} " + (f"{op.cout}" if dw else f"{op.cin}->{op.cout}")
            out.append({"op": n, "conv": "dw " + conv if dw else conv,
                        "fwd": _row(op.route_f, ("family", "name", "timer", "tiles", "work", "zero", "ldk")),
                        "dgrad": _row(op.route_d, ("family", "name", "timer", "work", "zero", "ldk", "bnout",
                                                   "fallback")),
                        "wgrad": _row(op.route_w, ("family", "name", "timer", "work", "splits"))})
    return out


def main():
    tab = {f"{arch} {N}x{H}x{W} {math}": table(build(arch, N, H, W, math))
           for arch, N, H, W, maths in PROGRAMS for math in maths}
    with open(os.path.join(HERE, "engine_routes.json"), "w") as fh:
        fh.write("{\n" + ",\n".join(
            json.dumps(key) + ": [\n" + ",\n".join(" " + json.dumps(row, sort_keys=True) for row in rows) + "\n]"
            for key, rows in tab.items()) + "\n}\n")
    print("engine_routes.json written")


if __name__ == "__main__":
    main()
