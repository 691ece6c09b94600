"""Time a one-logit training step on one MI355X: the fused BinarySegLoss against nn.BCEWithLogitsLoss on the logits.

    python tools/binarybench.py [--bs 32] [--hw 256 512] [--steps 20] [--rounds 3] [--out profiles/binary_bench.txt]

MobileNetV2UNet(1) in train(), one device-resident batch with a binary mask, seg_amd.Adam, at conv math f32 and
bf16io:
  (A) fused:  compute_loss with seg_amd.BinarySegLoss() -- seg_bce_upsample_loss / _grad: neither the full-resolution
              logits nor their gradient are stored (the gradient kernel writes one fp32 per pixel);
  (B) logits: nn.BCEWithLogitsLoss()(model(x)[:, 0], t.float()) -- the only way to train this model without the
              feature, and the baseline.
A step is zero_grad, loss, backward, optimizer step; `--steps` of them are timed with the host clock between two
device synchronises; A and B alternate inside every round (each finds its recorded plan again).  Peak memory is
torch.cuda.max_memory_allocated over each configuration's warm-up, taken while only its own plan exists.  Then the
kernels alone: seg_bce_upsample_loss / _grad at C = 1 beside seg_ce_upsample_loss / _grad at C = 10 on the same
pixel count (device events over back-to-back launches).  Prints everything and writes it to --out.  Needs an
MI355X: there is no CPU path.
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

from seg_amd import Adam, BinarySegLoss, MobileNetV2UNet, deterministic_init  # noqa: E402
from seg_amd.detinit import synthetic_scene  # noqa: E402
from seg_amd.engine import release_plans, set_conv_math  # noqa: E402
from seg_amd.train import compute_loss  # noqa: E402

DEV = "cuda"


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


def launches(fn, n=50, rounds=3):
    for _ in range(10):
        fn()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / n)
    return statistics.median(us), min(us), max(us)


def kernel_times(N, H, W):
    """seg_bce_* at C = 1 beside seg_ce_* at C = 10: low-resolution rows [N, H, W], output (2H, 2W)."""
    from seg_amd._lib import call, query
    s = torch.cuda.current_stream().cuda_stream
    Ho, Wo = 2 * H, 2 * W
    pix = N * Ho * Wo
    g = torch.Generator().manual_seed(5)
    gout = torch.ones(1, device=DEV)
    lines = []
    for sfx, dt in (("", torch.float32), ("_bf16io", torch.bfloat16)):
        low1 = (torch.randn(N * H * W, 4, generator=g) * 2).to(DEV, dt)
        low10 = (torch.randn(N * H * W, 12, generator=g) * 2).to(DEV, dt)
        t1 = torch.randint(0, 2, (N, Ho, Wo), generator=g).to(DEV)
        t10 = torch.randint(0, 10, (N, Ho, Wo), generator=g).to(DEV)
        st8, st3 = torch.empty(8, device=DEV), torch.empty(3, device=DEV)
        wb = torch.empty(query("seg_bce_workspace_floats", pix), device=DEV)
        wc = torch.empty(query("seg_ce_workspace_floats", pix), device=DEV)
        d1 = torch.empty(pix, device=DEV)               # one fp32 per pixel, in both maths
        d10 = torch.empty(pix * 12, device=DEV, dtype=dt)
        fns = {
            "seg_bce_upsample_loss": lambda: call("seg_bce_upsample_loss" + sfx, low1.data_ptr(), 4, N, H, W, 1,
                                                  t1.data_ptr(), Ho, Wo, -100, 1.0, 1.0, 0.0, 0.0, 1.0,
                                                  wb.data_ptr(), st8.data_ptr(), s),
            "seg_bce_upsample_grad": lambda: call("seg_bce_upsample_grad" + sfx, low1.data_ptr(), 4, N, H, W, 1,
                                                  t1.data_ptr(), Ho, Wo, -100, 1.0, 1.0, 0.0, 0.0, gout.data_ptr(),
                                                  st8.data_ptr(), d1.data_ptr(), s),
            "seg_ce_upsample_loss (C = 10)": lambda: call("seg_ce_upsample_loss" + sfx, low10.data_ptr(), 12, N, H,
                                                          W, 10, t10.data_ptr(), Ho, Wo, -100, wc.data_ptr(),
                                                          st3.data_ptr(), s),
            "seg_ce_upsample_grad (C = 10)": lambda: call("seg_ce_upsample_grad" + sfx, low10.data_ptr(), 12, N, H,
                                                          W, 10, t10.data_ptr(), Ho, Wo, -100, gout.data_ptr(),
                                                          st3.data_ptr(), d10.data_ptr(), 12, s)}
        es = 2 if sfx else 4
        written = {"seg_bce_upsample_grad": pix * 4, "seg_ce_upsample_grad (C = 10)": pix * 12 * es}
        for k, fn in fns.items():
            med, lo, hi = launches(fn)
            extra = f"   writes {written[k] / 2**20:.0f} MiB" if k in written else ""
            lines.append(f"  {'bf16io' if sfx else 'f32':7s}{k:32s} {med:8.1f} us ({lo:.1f}..{hi:.1f}){extra}")
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
        raise SystemExit("binarybench.py needs an MI355X")
    H, W = a.hw
    x, y = (t.to(DEV) for t in synthetic_scene(a.bs, H, W, 4, seed=100))
    y = (y == 1).long()  # one class of the scene against the rest
    yf = y.float()
    plane = a.bs * H * W * 4
    lines = [f"one-logit training step, one MI355X: MobileNetV2UNet(1) train(), one resident batch {a.bs}x3x{H}x{W}, "
             f"seg_amd.Adam, ms per step over {a.steps} steps (host clock, device synchronise at both ends), warm-up "
             "of each;", "(A) fused seg_amd.BinarySegLoss(), (B) nn.BCEWithLogitsLoss on the model's logits; peak = "
             f"max_memory_allocated with only that configuration's plan alive; N*Ho*Wo*4 B = {plane / 2**20:.0f} MiB"]
    fused, bce = BinarySegLoss(), nn.BCEWithLogitsLoss()
    for math in ("f32", "bf16io"):
        model = deterministic_init(MobileNetV2UNet(1), seed=11).to(DEV).train()
        set_conv_math(model, math)
        opt = Adam(model.parameters(), lr=1.5e-4)
        modes = {"A fused": lambda: compute_loss(model, fused, x, y), "B logits": lambda: bce(model(x)[:, 0], yf)}
        peak = {}
        for k, fn in modes.items():  # each alone first: its own peak
            _, peak[k], _ = steps(model, opt, fn, 2)
            release_plans(model)
            torch.cuda.empty_cache()
        for fn in modes.values():    # ... then both plans recorded and kept
            steps(model, opt, fn, 2)
        ms, loss = {k: [] for k in modes}, {}
        for _ in range(a.rounds):
            for k, fn in modes.items():
                dt, _, loss[k] = steps(model, opt, fn, a.steps)
                ms[k].append(1e3 * dt)
        for k in modes:
            lines.append(f"{math:7s}{k:10s} " + "  ".join(f"{v:7.2f}" for v in ms[k])
                         + f"  ms   median {statistics.median(ms[k]):7.2f}  spread {min(ms[k]):.2f}..{max(ms[k]):.2f}"
                         + f"   peak {peak[k] / 2**20:8.0f} MiB   last loss {loss[k]:.4f}")
        ma, mb = statistics.median(ms["A fused"]), statistics.median(ms["B logits"])
        lines.append(f"{math:7s}logits / fused = {mb / ma:.3f}x step time; peak B - A = "
                     f"{(peak['B logits'] - peak['A fused']) / 2**20:.0f} MiB "
                     f"({(peak['B logits'] - peak['A fused']) / plane:.2f} x N*Ho*Wo*4 B)")
        release_plans(model)
        del model, opt
        torch.cuda.empty_cache()
    lines.append(f"the kernels alone, {a.bs}x{H // 2}x{W // 2} low-resolution rows to {a.bs}x{H}x{W}, device events "
                 "over 50 launches x 3 rounds, median (min..max):")
    lines += kernel_times(a.bs, H // 2, W // 2)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
