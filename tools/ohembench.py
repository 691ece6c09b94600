"""Time a training step with a seg_amd.OhemCELoss on one MI355X: fused against the logits path, and beside plain CE.

    python tools/ohembench.py [--bs 32] [--hw 256 512] [--steps 20] [--rounds 5] [--out profiles/ohem_bench.txt]

MobileNetV2UNet(10) in train(), one device-resident batch of a synthetic road scene, seg_amd.Adam, at conv math f32
and bf16io:
  (a) OhemCELoss(0.7, 1/16) fused: compute_loss -> model.forward_loss (seg_ohem_upsample_loss / _grad);
  (b) the same criterion on the logits path: criterion(model(x), t) -- full-resolution NCHW fp32 logits, the
      per-pixel losses, a topk over them and the masked mean in torch ops, autograd's temporaries and a full-resolution
      gradient;
  (c) plain nn.CrossEntropyLoss() fused;
  (d) OhemCELoss(thresh -> 0, 1/16) fused: no pixel passes the threshold, so the floor selects and the two refine
      passes of the radix select do their work (in (a) they return at once whenever 1/16 of the pixels are above tau).
A step is train_one_epoch's inner step: zero_grad, compute_loss, backward, _step_and_loss (the optimizer step and
loss.item()).  Each figure: `--steps` steps between two device events, after a warm-up that records the tapes; the
variants alternate inside every one of `--rounds` rounds; median and min..max over the rounds.  Every variant trains
its own model on the one batch, so the share of pixels (a) keeps falls as its model learns: the last step's #kept is
printed.  Peak memory is torch.cuda.max_memory_allocated over a variant's timed steps (every variant's plans stay
resident, so the differences are what a step allocates on top).  Not measured here: more than one GPU, and
convergence of a full run.
Needs an MI355X: there is no CPU path.
"""
import argparse
import math
import os
import statistics
import sys

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "team02-objectdetection_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import seg_amd  # noqa: E402
from seg_amd import engine, train  # noqa: E402
from seg_amd.detinit import synthetic_scene  # noqa: E402

DEV = "cuda"
C = 10


def stepper(conv_math, crit, fused, x, y):
    """One variant: its own model and optimizer; returns (step function, release function, #kept of the last step)."""
    model = seg_amd.deterministic_init(seg_amd.MobileNetV2UNet(C), seed=11).to(DEV).train()
    engine.set_conv_math(model, conv_math)
    opt = seg_amd.Adam(model.parameters(), lr=1.5e-4)
    loss_fn = (lambda: train.compute_loss(model, crit, x, y)) if fused else (lambda: crit(model(x), y))

    def step():
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        return train._step_and_loss(model, x, opt, loss, None)

    def kept():
        st = model.__dict__.get("_segamd_last_stats")
        return int(st[4].item()) if st is not None and st.numel() == 6 else None

    return step, lambda: engine.release_plans(model), kept


def timed(fn, steps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        lv = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps, torch.cuda.max_memory_allocated(), lv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=(256, 512))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ohembench.py needs an MI355X")
    H, W = a.hw
    x, y = (t.to(DEV) for t in synthetic_scene(a.bs, H, W, C, seed=100))
    ohem = seg_amd.OhemCELoss(0.7, 1 / 16).to(DEV)
    floor = seg_amd.OhemCELoss(math.exp(-60.0), 1 / 16).to(DEV)
    plain = nn.CrossEntropyLoss()
    pixels = a.bs * H * W
    lines = [f"training step, one MI355X: MobileNetV2UNet({C}) train(), one resident batch {a.bs}x3x{H}x{W} "
             f"({pixels} pixels), seg_amd.Adam; ms per step (zero_grad, loss, backward, optimizer step, loss.item()), "
             f"{a.steps} steps between device events, median (min..max) over {a.rounds} interleaved rounds; peak = "
             "torch.cuda.max_memory_allocated over the timed steps",
             "(a) OhemCELoss(0.7, 1/16) fused, (b) the same criterion on full-resolution logits, (c) plain "
             "nn.CrossEntropyLoss fused, (d) OhemCELoss(e^-60, 1/16) fused: the floor selects, the refine passes run"]
    for conv_math in ("f32", "bf16io"):
        variants = {"a OHEM fused": stepper(conv_math, ohem, True, x, y),
                    "b OHEM logits": stepper(conv_math, ohem, False, x, y),
                    "c plain CE fused": stepper(conv_math, plain, True, x, y),
                    "d OHEM fused, floor": stepper(conv_math, floor, True, x, y)}
        for fn, _, _ in variants.values():
            for _ in range(3):
                fn()
        ms, peak, loss = {k: [] for k in variants}, {}, {}
        for _ in range(a.rounds):
            for k, (fn, _, _) in variants.items():
                dt, pk, lv = timed(fn, a.steps)
                ms[k].append(dt)
                peak[k], loss[k] = pk, lv
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, (_, _, kept) in variants.items():
            n = kept()
            lines.append(f"{conv_math:7s}{k:22s} median {med[k]:7.2f} ms  ({min(ms[k]):.2f}..{max(ms[k]):.2f})   "
                         f"peak {peak[k] / 2**20:8.0f} MiB   last loss {loss[k]:.4f}"
                         + (f"   last #kept {n} ({100.0 * n / pixels:.1f} %)" if n is not None else ""))
        lines.append(f"{conv_math:7s}logits / fused = {med['b OHEM logits'] / med['a OHEM fused']:.2f}x step time, "
                     f"{(peak['b OHEM logits'] - peak['a OHEM fused']) / 2**20:.0f} MiB more at peak "
                     f"(N*C*Ho*Wo*4 = {a.bs * C * H * W * 4 / 2**20:.0f} MiB); OHEM fused - plain CE fused = "
                     f"{1e3 * (med['a OHEM fused'] - med['c plain CE fused']):+.0f} us per step (threshold mode), "
                     f"{1e3 * (med['d OHEM fused, floor'] - med['c plain CE fused']):+.0f} us (floor mode); the "
                     f"largest min..max spread is {1e3 * max(max(v) - min(v) for v in ms.values()):.0f} us")
        for _, release, _ in variants.values():
            release()
        del variants
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
