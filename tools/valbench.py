"""Time a validation pass on one MI355X: the fused path against the logits path.

    python tools/valbench.py [--bs 32] [--hw 256 512] [--batches 20] [--rounds 3] [--out profiles/val_bench.txt]

MobileNetV2UNet(10) in eval(), `--batches` device-resident batches of synthetic road scenes, at conv math
f32 and bf16io:
  (a) fused:  seg_amd.validate() -- per batch one forward tape ending in seg_ce_upsample_eval (loss + argmax +
              confusion matrix from the low-resolution logits), one host wait per pass;
  (b) logits: per batch model(x) (full-resolution NCHW fp32 logits), F.cross_entropy, argmax and
              seg_amd.detinit.miou (host bincount) -- the only way to evaluate before forward_metrics existed.
Both compute the same quantities (checked: equal loss within 1e-5, equal mIoU within 1e-3 -- argmax near-ties).
A pass is timed with the host clock around work that ends in a device synchronise; one warm-up pass of each
(it records the tapes), then the two alternate inside every round.  Prints img/s per round, the medians and
the ratio, then the eval kernel beside the loss kernel alone (kernel_times), and writes the same text to --out.
Needs an MI355X: there is no CPU path.
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "team02-objectdetection_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from seg_amd import MobileNetV2UNet, deterministic_init, validate  # noqa: E402
from seg_amd.detinit import miou, synthetic_scene  # noqa: E402
from seg_amd.engine import release_plans, set_conv_math  # noqa: E402

DEV = "cuda"
C = 10


def logits_pass(model, loader):
    """(mean batch loss, mIoU) the way tests/test_gpu_miou.py evaluates."""
    model.eval()
    losses, preds, targets = [], [], []
    with torch.no_grad():
        for x, y in loader:
            out = model(x)
            losses.append(F.cross_entropy(out, y))
            preds.append(out.argmax(1).cpu())
            targets.append(y.cpu())
    loss = torch.stack(losses).mean().item()
    return loss, miou(torch.cat(preds), torch.cat(targets), C)


def fused_pass(model, loader):
    r = validate(model, loader, nn.CrossEntropyLoss(), DEV, progress=False)
    return r["loss"], r["miou"]


def kernel_times(bs, H, W, scene_labels, launches=50, rounds=3):
    """The eval kernel beside the loss kernel alone (device events over `launches` back-to-back launches, the two
    alternating in every round), fp32 low-resolution logits, on two label / logit fields: random logits with
    uniform labels (counts spread over all C*C bins), and one dominant class with the road-scene labels (nearly
    every pixel of a block in one bin: the most contended LDS atomics)."""
    from seg_amd._lib import call, query
    h, w, ld = H // 2, W // 2, 12
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    spread = torch.randn(bs * h * w, ld, generator=g).to(DEV)
    one = spread.clone()
    one[:, 2] += 8.0
    fields = {"uniform labels, random logits": (spread, torch.randint(0, C, (bs, H, W), generator=g).to(DEV)),
              "road-scene labels, one predicted class": (one, scene_labels)}
    work = torch.empty(query("seg_ce_workspace_floats", bs * H * W), device=DEV)
    out3 = torch.empty(3, device=DEV)
    conf = torch.zeros(C * C, dtype=torch.int64, device=DEV)
    lines = []
    for name, (low, y) in fields.items():
        fns = {"loss": lambda: call("seg_ce_upsample_loss", low.data_ptr(), ld, bs, h, w, C, y.data_ptr(), H, W, -100,
                                    work.data_ptr(), out3.data_ptr(), s),
               "eval": lambda: call("seg_ce_upsample_eval", low.data_ptr(), ld, bs, h, w, C, y.data_ptr(), H, W, -100,
                                    work.data_ptr(), out3.data_ptr(), conf.data_ptr(), s)}
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
        lines.append(f"{name}: " + "; ".join(
            f"{k} {statistics.median(v):.1f} us ({min(v):.1f}..{max(v):.1f})" for k, v in us.items()))
    return lines


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=(256, 512))
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=2, help="distinct scene batches generated (then repeated)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("valbench.py needs an MI355X")
    H, W = a.hw
    scenes = [synthetic_scene(a.bs, H, W, C, seed=100 + k) for k in range(min(a.distinct, a.batches))]
    loader = [tuple(t.to(DEV).clone() for t in scenes[k % len(scenes)]) for k in range(a.batches)]
    images = a.bs * a.batches
    lines = [f"validation pass, one MI355X: MobileNetV2UNet({C}) eval(), {a.batches} resident batches of "
             f"{a.bs}x3x{H}x{W}, img/s over a whole pass (host clock, device synchronise at both ends),",
             "one warm-up pass of each, then fused (validate / forward_metrics) and logits (model(x) + "
             "F.cross_entropy + argmax + detinit.miou) alternate in every round"]
    mismatch = []
    for math in ("f32", "bf16io"):
        model = deterministic_init(MobileNetV2UNet(C), seed=11, random_running_stats=True).to(DEV).eval()
        set_conv_math(model, math)
        (_, (lf, mf)), (_, (ll, ml)) = timed(fused_pass, model, loader), timed(logits_pass, model, loader)
        if not (abs(lf - ll) <= 1e-5 * abs(ll) and abs(mf - ml) <= 1e-3):
            mismatch.append(math)
        rates = {"fused": [], "logits": []}
        for _ in range(a.rounds):
            for name, fn in (("fused", fused_pass), ("logits", logits_pass)):
                dt, _ = timed(fn, model, loader)
                rates[name].append(images / dt)
        med = {k: statistics.median(v) for k, v in rates.items()}
        lines.append(f"{math}: loss {lf:.6f} (fused) {ll:.6f} (logits), mIoU {mf:.6f} / {ml:.6f}")
        for name in ("fused", "logits"):
            lines.append(f"{math:7s}{name:7s} " + "  ".join(f"{r:9.1f}" for r in rates[name])
                         + f"  img/s   median {med[name]:9.1f}  spread {min(rates[name]):.1f}..{max(rates[name]):.1f}")
        lines.append(f"{math:7s}fused / logits = {med['fused'] / med['logits']:.2f}x")
        release_plans(model)
        del model
        torch.cuda.empty_cache()
    lines.append(f"kernels alone, {a.bs}x{H}x{W} pixels from {H // 2}x{W // 2} fp32 logits (finalize launch included), "
                 "device events over 50 launches x 3 rounds, median (min..max):")
    lines += kernel_times(a.bs, H, W, loader[0][1])
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if mismatch:
        raise SystemExit(f"the two paths disagree at {mismatch}: the timings above compare different results")


if __name__ == "__main__":
    main()
