"""Time a training step with a seg_amd.SegLoss on one MI355X: fused against the logits path, and plain CE beside the
parent commit's.

    python tools/seglossbench.py [--bs 32] [--hw 256 512] [--steps 20] [--rounds 5] [--parent DIR]
                                 [--out profiles/seg_loss_bench.txt]

MobileNetV2UNet(10) in train(), one device-resident batch of a synthetic road scene, seg_amd.Adam, at conv math f32
and bf16io:
  (a) SegLoss(ce=1, dice=1, focal_gamma=2) fused: compute_loss -> model.forward_loss (seg_sl_upsample_loss / _grad);
  (b) the same criterion on the logits path: criterion(model(x), t) -- full-resolution NCHW fp32 logits, SegLoss's
      torch forward, autograd's temporaries and a full-resolution gradient;
  (c) plain nn.CrossEntropyLoss() fused, on this tree and (--parent: a checkout of the parent commit with its library
      built; its package is imported under another name and loads its own library) on the parent commit.
A step is train_one_epoch's inner step: zero_grad, compute_loss, backward, _step_and_loss (the optimizer step and
loss.item()).  Each figure: `--steps` steps between two device events, after a warm-up that records the tapes; the
variants alternate inside every one of `--rounds` rounds; median and min..max over the rounds.  Peak memory is
torch.cuda.max_memory_allocated over a variant's timed steps (every variant's plans stay resident, so the differences
are what a step allocates on top).  Not measured here: more than one GPU, and convergence.
Needs an MI355X: there is no CPU path.
"""
import argparse
import importlib
import importlib.util
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
from seg_amd.detinit import synthetic_scene  # noqa: E402

DEV = "cuda"
C = 10


def load_parent(path):
    """The parent checkout's seg_amd package under another name: its engine, its _lib.py, its own library."""
    pkg = os.path.join(path, "team02-objectdetection_amd", "seg_amd")
    spec = importlib.util.spec_from_file_location("seg_amd_parent", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["seg_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def stepper(pkg, math, crit, fused, x, y):
    """One variant: its own model and optimizer from package `pkg`; returns (step function, release function)."""
    engine = importlib.import_module(pkg.__name__ + ".engine")
    train = importlib.import_module(pkg.__name__ + ".train")
    model = pkg.deterministic_init(pkg.MobileNetV2UNet(C), seed=11).to(DEV).train()
    engine.set_conv_math(model, math)
    opt = pkg.Adam(model.parameters(), lr=1.5e-4)
    loss_fn = (lambda: train.compute_loss(model, crit, x, y)) if fused else (lambda: crit(model(x), y))

    def step():
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        return train._step_and_loss(model, x, opt, loss, None)

    return step, lambda: engine.release_plans(model)


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
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seglossbench.py needs an MI355X")
    H, W = a.hw
    x, y = (t.to(DEV) for t in synthetic_scene(a.bs, H, W, C, seed=100))
    seg = seg_amd.SegLoss(ce=1.0, dice=1.0, focal_gamma=2.0).to(DEV)
    plain = nn.CrossEntropyLoss()
    parent = load_parent(a.parent) if a.parent else None
    if parent is not None:
        assert not hasattr(parent, "SegLoss") and parent._lib is not seg_amd._lib
    lines = [f"training step, one MI355X: MobileNetV2UNet({C}) train(), one resident batch {a.bs}x3x{H}x{W}, "
             f"seg_amd.Adam; ms per step (zero_grad, loss, backward, optimizer step, loss.item()), {a.steps} steps "
             f"between device events, median (min..max) over {a.rounds} interleaved rounds; peak = "
             "torch.cuda.max_memory_allocated over the timed steps",
             "(a) SegLoss(ce=1, dice=1, focal_gamma=2) fused, (b) the same criterion on full-resolution logits, "
             "(c) plain nn.CrossEntropyLoss fused on this tree" + (" and on the parent commit" if parent else
                                                                    " (parent commit not given: not measured)")]
    for math in ("f32", "bf16io"):
        variants = {"a SegLoss fused": stepper(seg_amd, math, seg, True, x, y),
                    "b SegLoss logits": stepper(seg_amd, math, seg, False, x, y),
                    "c plain CE, this tree": stepper(seg_amd, math, plain, True, x, y)}
        if parent is not None:
            variants["c plain CE, parent"] = stepper(parent, math, plain, True, x, y)
        for fn, _ in variants.values():
            for _ in range(3):
                fn()
        ms, peak, loss = {k: [] for k in variants}, {}, {}
        for _ in range(a.rounds):
            for k, (fn, _) in variants.items():
                dt, pk, lv = timed(fn, a.steps)
                ms[k].append(dt)
                peak[k], loss[k] = pk, lv
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in variants:
            lines.append(f"{math:7s}{k:24s} median {med[k]:7.2f} ms  ({min(ms[k]):.2f}..{max(ms[k]):.2f})   "
                         f"peak {peak[k] / 2**20:8.0f} MiB   last loss {loss[k]:.4f}")
        lines.append(f"{math:7s}logits / fused = {med['b SegLoss logits'] / med['a SegLoss fused']:.2f}x step time, "
                     f"{(peak['b SegLoss logits'] - peak['a SegLoss fused']) / 2**20:.0f} MiB more at peak "
                     f"(N*C*Ho*Wo*4 = {a.bs * C * H * W * 4 / 2**20:.0f} MiB); SegLoss fused / plain CE fused = "
                     f"{med['a SegLoss fused'] / med['c plain CE, this tree']:.3f}x")
        if parent is not None:
            p = ms["c plain CE, parent"]
            lines.append(f"{math:7s}plain CE: this tree {med['c plain CE, this tree']:.2f} ms, parent "
                         f"{med['c plain CE, parent']:.2f} ms (its rounds {min(p):.2f}..{max(p):.2f})")
        for _, release in variants.values():
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
