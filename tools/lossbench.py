"""Time a training step with a weighted, smoothed criterion on one MI355X: fused against the logits path.

    python tools/lossbench.py [--bs 32] [--hw 256 512] [--steps 20] [--rounds 3] [--out profiles/loss_bench.txt]

MobileNetV2UNet(10) in train(), one device-resident batch of a synthetic road scene, seg_amd.Adam, at conv math
f32 and bf16io:
  (a) plain fused:    nn.CrossEntropyLoss()                                   through model.forward_loss;
  (b) weighted fused: nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)      through model.forward_loss
                      (seg_cew_upsample_loss / _grad: no full-resolution logits);
  (c) weighted logits: the same criterion as criterion(model(x), t) -- full-resolution NCHW fp32 logits, aten's
                      log-softmax + NLL, a full-resolution gradient: the only way before the kernels took the options.
A step is zero_grad, loss, backward, optimizer step; `--steps` of them are timed with the host clock between two
device synchronises, after a warm-up that records the tapes; the three alternate inside every round.  Peak memory
is torch.cuda.max_memory_allocated over the timed steps of (b) and (c).  Then the new loss, grad and eval kernels
beside the plain ones alone (device events over back-to-back launches).  Prints everything and writes it to --out.
Needs an MI355X: there is no CPU path.
"""
import argparse
import os
import statistics
import sys
import time

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "team02-objectdetection_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from seg_amd import Adam, MobileNetV2UNet, class_weights, deterministic_init  # noqa: E402
from seg_amd.detinit import synthetic_scene  # noqa: E402
from seg_amd.engine import release_plans, set_conv_math  # noqa: E402
from seg_amd.train import compute_loss  # noqa: E402

DEV = "cuda"
C = 10


def steps(model, opt, loss_fn, n):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(n):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, torch.cuda.max_memory_allocated(), float(loss.detach())


def kernel_times(bs, H, W, y, w, launches=50, rounds=3):
    """The weighted / smoothed kernels beside the plain ones alone, fp32 and bf16 low-resolution logits."""
    from seg_amd._lib import call, query
    h, wd, ld = H // 2, W // 2, 12
    s = torch.cuda.current_stream().cuda_stream
    low32 = torch.randn(bs * h * wd, ld, generator=torch.Generator().manual_seed(1)).to(DEV)
    work = torch.empty(query("seg_cew_workspace_floats", bs * H * W), device=DEV)
    out = torch.empty(4, device=DEV)
    g = torch.ones(1, device=DEV)
    conf = torch.zeros(C * C, dtype=torch.int64, device=DEV)
    lines = []
    for sfx, low in (("", low32), ("_bf16io", low32.to(torch.bfloat16))):
        dh = torch.empty(bs * H * W, ld, device=DEV, dtype=low.dtype)
        head = (low.data_ptr(), ld, bs, h, wd, C, y.data_ptr(), H, W, -100)
        opt = (w.data_ptr(), 0.1)
        fns = {
            "loss": lambda: call("seg_ce_upsample_loss" + sfx, *head, work.data_ptr(), out.data_ptr(), s),
            "loss_w": lambda: call("seg_cew_upsample_loss" + sfx, *head, *opt, 0, work.data_ptr(), out.data_ptr(), s),
            "eval": lambda: call("seg_ce_upsample_eval" + sfx, *head, work.data_ptr(), out.data_ptr(),
                                 conf.data_ptr(), s),
            "eval_w": lambda: call("seg_cew_upsample_eval" + sfx, *head, *opt, 0, work.data_ptr(), out.data_ptr(),
                                   conf.data_ptr(), s),
            "grad": lambda: call("seg_ce_upsample_grad" + sfx, *head, g.data_ptr(), out.data_ptr(), dh.data_ptr(),
                                 ld, s),
            "grad_w": lambda: call("seg_cew_upsample_grad" + sfx, *head, *opt, g.data_ptr(), out.data_ptr(),
                                   dh.data_ptr(), ld, s)}
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
        lines.append(f"{'fp32' if not sfx else 'bf16'} logits: " + "; ".join(
            f"{k} {statistics.median(v):.1f} us ({min(v):.1f}..{max(v):.1f})" for k, v in us.items()))
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
        raise SystemExit("lossbench.py needs an MI355X")
    H, W = a.hw
    x, y = (t.to(DEV) for t in synthetic_scene(a.bs, H, W, C, seed=100))
    w = class_weights(torch.bincount(y.reshape(-1).cpu(), minlength=C), clip=10.0).to(DEV)
    plain = nn.CrossEntropyLoss()
    crit = nn.CrossEntropyLoss(weight=w, label_smoothing=0.1).to(DEV)
    lines = [f"training step, one MI355X: MobileNetV2UNet({C}) train(), one resident batch {a.bs}x3x{H}x{W}, seg_amd.Adam, "
             f"ms per step over {a.steps} steps (host clock, device synchronise at both ends), one warm-up of each;",
             "(a) plain fused, (b) weighted + smoothed fused, (c) the same criterion on full-resolution logits; "
             f"class weights {[round(v, 3) for v in w.tolist()]}"]
    for math in ("f32", "bf16io"):
        model = deterministic_init(MobileNetV2UNet(C), seed=11).to(DEV).train()
        set_conv_math(model, math)
        opt = Adam(model.parameters(), lr=1.5e-4)
        paths = {"a plain fused": lambda: compute_loss(model, plain, x, y),
                 "b weighted fused": lambda: compute_loss(model, crit, x, y),
                 "c weighted logits": lambda: crit(model(x), y)}
        for fn in paths.values():
            steps(model, opt, fn, 2)
        ms, peak, loss = {k: [] for k in paths}, {}, {}
        for _ in range(a.rounds):
            for k, fn in paths.items():
                dt, pk, lv = steps(model, opt, fn, a.steps)
                ms[k].append(1e3 * dt)
                peak[k], loss[k] = pk, lv
        for k in paths:
            lines.append(f"{math:7s}{k:18s} " + "  ".join(f"{v:7.2f}" for v in ms[k])
                         + f"  ms   median {statistics.median(ms[k]):7.2f}  spread {min(ms[k]):.2f}..{max(ms[k]):.2f}"
                         + f"   peak {peak[k] / 2**20:8.0f} MiB   last loss {loss[k]:.4f}")
        mb, mc = statistics.median(ms["b weighted fused"]), statistics.median(ms["c weighted logits"])
        lines.append(f"{math:7s}logits / fused = {mc / mb:.2f}x step time, "
                     f"{(peak['c weighted logits'] - peak['b weighted fused']) / 2**20:.0f} MiB more at peak "
                     f"(N*C*Ho*Wo*4 = {a.bs * C * H * W * 4 / 2**20:.0f} MiB)")
        release_plans(model)
        del model, opt
        torch.cuda.empty_cache()
    lines.append(f"kernels alone, {a.bs}x{H}x{W} pixels from {H // 2}x{W // 2} logits (loss / eval: finalize launch "
                 "included), weights + smoothing 0.1 (_w) beside the plain ones, device events over 50 launches x 3 "
                 "rounds, median (min..max):")
    lines += kernel_times(a.bs, H, W, y, w)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
