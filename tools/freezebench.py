"""Time a fine-tuning step on one MI355X: backbone frozen (seg_amd.freeze) against the full step.

    python tools/freezebench.py [--bs 32] [--hw 256 512] [--steps 20] [--rounds 3] [--out profiles/freeze_bench.txt]

MobileNetV2UNet(10) in train(), one device-resident batch of a synthetic road scene, seg_amd.Adam, at conv math f32
and bf16io:
  (a) frozen: seg_amd.freeze(model) -- no gradients for the backbone, its BatchNorm layers on their running
              statistics; the backward stops at up1's first conv (engine.grad_frontier);
  (b) full:   the same model after seg_amd.unfreeze(model).
A step is zero_grad, fused loss, backward, optimizer step; `--steps` of them are timed with the host clock between
two device synchronises; the two alternate inside every round (freeze / unfreeze between them: each finds its
recorded plan again).  Peak memory is torch.cuda.max_memory_allocated over each configuration's warm-up, taken while
only its own plan exists.  Then seg_bn_frozen_backward beside seg_bn_backward alone, on the widest-image and the
widest-channel BatchNorm layer of the model (device events over back-to-back launches).  Prints everything and
writes it to --out.  Needs an MI355X: there is no CPU path.
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "team02-objectdetection_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from seg_amd import Adam, MobileNetV2UNet, deterministic_init, freeze, unfreeze  # noqa: E402
from seg_amd.detinit import synthetic_scene  # noqa: E402
from seg_amd.engine import release_plans, set_conv_math  # noqa: E402

DEV = "cuda"
C = 10


def steps(model, opt, x, y, n):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(n):
        opt.zero_grad()
        loss = model.forward_loss(x, y)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, torch.cuda.max_memory_allocated(), float(loss.detach())


def kernel_times(layers, launches=50, rounds=3):
    """seg_bn_frozen_backward (affine gradients + dY; dY alone) beside seg_bn_backward, fp32 and bf16 storage."""
    from seg_amd._lib import call, query
    s = torch.cuda.current_stream().cuda_stream
    lines = []
    for M, Cc in layers:
        g = torch.Generator().manual_seed(M % 1009 + Cc)
        y32 = (torch.randn(M, Cc, generator=g) * 2 + 0.5).to(DEV)
        d32 = torch.randn(M, Cc, generator=g).to(DEV)
        v = [t.to(DEV) for t in (torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.2,
                                 torch.rand(Cc, generator=g) + 0.5, torch.rand(Cc, generator=g) + 0.5,
                                 torch.randn(Cc, generator=g) * 0.3)]
        gamma, mean, var, scale, shift = v
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        gw, gb = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
        work = torch.zeros(query("seg_chan_workspace_floats", M, Cc) + 3 * Cc, device=DEV)
        for sfx, y, d in (("", y32, d32), ("_bf16io", y32.to(torch.bfloat16), d32.to(torch.bfloat16))):
            dy = torch.empty_like(y)
            head = (d.data_ptr(), Cc, y.data_ptr(), Cc, M, Cc)
            frozen = (*head, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), var.data_ptr(), 1e-5, 2)
            fns = {
                "train (seg_bn_backward)": lambda: call(
                    "seg_bn_backward" + sfx, *head, gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                    scale.data_ptr(), shift.data_ptr(), 2, gw.data_ptr(), gb.data_ptr(), work.data_ptr(),
                    dy.data_ptr(), Cc, s),
                "frozen": lambda: call("seg_bn_frozen_backward" + sfx, *frozen, gw.data_ptr(), gb.data_ptr(),
                                       work.data_ptr(), dy.data_ptr(), Cc, s),
                "frozen, no affine": lambda: call("seg_bn_frozen_backward" + sfx, *frozen, None, None, None,
                                                  dy.data_ptr(), Cc, s)}
            us = {k: [] for k in fns}
            for fn in fns.values():
                for _ in range(10):
                    fn()
            for _ in range(rounds):
                for k, fn in fns.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(launches):
                        fn()
                    b.record()
                    b.synchronize()
                    us[k].append(1e3 * a.elapsed_time(b) / launches)
            es = 2 if sfx else 4
            lines.append(f"{M} x {Cc} {'bf16' if sfx else 'fp32'}: " + "; ".join(
                f"{k} {statistics.median(t):.1f} us ({min(t):.1f}..{max(t):.1f})" for k, t in us.items())
                + f"   [3|Y| at the frozen median: {3 * M * Cc * es / statistics.median(us['frozen']) / 1e6:.2f} TB/s]")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=(256, 512))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("freezebench.py needs an MI355X")
    H, W = a.hw
    x, y = (t.to(DEV) for t in synthetic_scene(a.bs, H, W, C, seed=100))
    lines = [f"fine-tuning step, one MI355X: MobileNetV2UNet({C}) train(), one resident batch {a.bs}x3x{H}x{W}, "
             f"seg_amd.Adam, fused loss, ms per step over {a.steps} steps (host clock, device synchronise at both "
             "ends), warm-up of each;", "(a) backbone frozen (parameters and BatchNorm statistics), (b) full step; "
             "peak = max_memory_allocated with only that configuration's plan alive"]
    for math in ("f32", "bf16io"):
        model = deterministic_init(MobileNetV2UNet(C), seed=11).to(DEV).train()
        set_conv_math(model, math)
        opt = Adam(model.parameters(), lr=1.5e-4)
        modes = {"a frozen": lambda: freeze(model), "b full": lambda: unfreeze(model)}
        peak = {}
        for k, enter in modes.items():  # each alone first: its own peak
            enter()
            _, peak[k], _ = steps(model, opt, x, y, 2)
            release_plans(model)
            torch.cuda.empty_cache()
        for enter in modes.values():    # ... then both plans recorded and kept
            enter()
            steps(model, opt, x, y, 2)
        ms, loss = {k: [] for k in modes}, {}
        for _ in range(a.rounds):
            for k, enter in modes.items():
                enter()
                dt, _, loss[k] = steps(model, opt, x, y, a.steps)
                ms[k].append(1e3 * dt)
        for k in modes:
            lines.append(f"{math:7s}{k:10s} " + "  ".join(f"{v:7.2f}" for v in ms[k])
                         + f"  ms   median {statistics.median(ms[k]):7.2f}  spread {min(ms[k]):.2f}..{max(ms[k]):.2f}"
                         + f"   peak {peak[k] / 2**20:8.0f} MiB   last loss {loss[k]:.4f}")
        mf, mu = statistics.median(ms["a frozen"]), statistics.median(ms["b full"])
        lines.append(f"{math:7s}full / frozen = {mu / mf:.2f}x step time")
        release_plans(model)
        del model, opt
        torch.cuda.empty_cache()
    layers = [(a.bs * (H // 2) * (W // 2), 32), (a.bs * (H // 32) * (W // 32), 1280)]
    lines.append("BatchNorm backward alone (ReLU6), frozen statistics (one pass) beside train mode (seg_bn_backward: "
                 "partials, finalize, apply), device events over 50 launches x 3 rounds, median (min..max):")
    lines += kernel_times(layers)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
