"""Time the weight averaging on one MI355X: seg_amd.EMA beside torch._foreach_lerp_.

    python tools/emabench.py [--steps 200] [--rounds 5] [--loop-steps 20] [--out profiles/ema_bench.txt]

The tensors are MobileNetV2UNet(10)'s real state: every floating-point state_dict entry (parameters and BatchNorm
running statistics), each tensor once.
  (a) EMA.update() (the pointer check and one seg_ema_update launch) beside torch._foreach_lerp_ over the same
      tensors into shadows of its own;
  (b) the seg_ema_update launch alone and the seg_ema_swap launch alone (table and chunk map already on the device);
      the swap is timed in pairs, so the model's weights are the same after every call;
  (c) a train_one_epoch-style loop on synthetic_batch (bs 32, 256x512, seg_amd.AdamW, fused CE) with and without
      `ema`: ms per step over `--loop-steps` steps per timing, from the host clock around a final synchronize.
Each figure of (a) and (b): `--steps` calls back to back between two device events (so a call that the host cannot
issue as fast as the device runs it is charged its host time), after a warm-up; the variants of a group alternate
inside every one of `--rounds` rounds; median and min..max over the rounds.  Needs an MI355X: there is no CPU path.
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

import seg_amd  # noqa: E402
from seg_amd import EMA, MobileNetV2UNet, decay_groups, deterministic_init, synthetic_batch  # noqa: E402
from seg_amd._lib import call  # noqa: E402
from seg_amd.optim import _CHUNK  # noqa: E402

DEV = "cuda"


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps


def group(title, fns, steps, rounds, unit="us"):
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn, steps))
    lines = [title]
    for k, t in us.items():
        lines.append(f"    {k:58s} median {statistics.median(t):8.1f} {unit}   ({min(t):.1f}..{max(t):.1f})")
    return lines, {k: statistics.median(t) for k, t in us.items()}


def loop_ms(model, opt, ema, batch, steps):
    """ms per step of `steps` train_one_epoch steps (the host clock around a final synchronize)."""
    loader = [batch] * steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seg_amd.train_one_epoch(model, loader, nn.CrossEntropyLoss(), opt, DEV, progress=False, ema=ema)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("emabench.py needs an MI355X")
    model = deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV).train()
    ema = EMA(model, decay=0.999)
    srcs = [s.detach() for s in ema._sources()]
    n = sum(s.numel() for s in srcs)
    lines = [f"weight averaging, one MI355X: MobileNetV2UNet(10), {len(ema.names)} floating-point state_dict entries, "
             f"{len(srcs)} tensors, {n} elements ({8 * n / 1e6:.0f} MB read + {4 * n / 1e6:.0f} MB written per "
             f"update, {8 * n / 1e6:.0f} + {8 * n / 1e6:.0f} MB per swap); us per call, {a.steps} calls back to back "
             f"between device events, median (min..max) over {a.rounds} interleaved rounds"]
    # (a) the update beside torch's foreach lerp
    theirs = [s.clone() for s in srcs]

    def foreach_lerp():
        torch._foreach_lerp_(theirs, srcs, 1e-3)

    la, ma = group("(a) one update of every shadow", {"seg_amd.EMA.update()": ema.update,
                                                      "torch._foreach_lerp_(shadows, tensors, 1 - decay)": foreach_lerp},
                   a.steps, a.rounds)
    lines += la
    # (b) the launches alone
    table, chunks = ema._table, ema._chunks
    stream = torch.cuda.current_stream().cuda_stream

    def update_launch():
        call("seg_ema_update", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], _CHUNK, 1e-3, None, stream)

    def swap_pair():
        call("seg_ema_swap", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], _CHUNK, stream)
        call("seg_ema_swap", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], _CHUNK, stream)

    lb, mb = group(f"(b) the launches alone ({chunks.shape[0]} blocks)",
                   {"seg_ema_update launch": update_launch, "seg_ema_swap launch, twice (there and back)": swap_pair},
                   a.steps, a.rounds)
    lines += lb
    # (c) the training loop with and without the average
    del theirs
    H, W = 256, 512
    batch = synthetic_batch(a.batch, H, W, 10, seed=111)
    batch = (batch[0].to(DEV), batch[1].to(DEV))
    opt = seg_amd.AdamW(decay_groups(model, 1e-2), lr=1e-4)
    for e in (None, ema, None, ema):  # warm-up: plan recording, allocator
        loop_ms(model, opt, e, batch, 3)
    ms = {"without ema": [], "with ema=EMA(model)": []}
    for _ in range(a.rounds):
        ms["without ema"].append(loop_ms(model, opt, None, batch, a.loop_steps))
        ms["with ema=EMA(model)"].append(loop_ms(model, opt, ema, batch, a.loop_steps))
    lines.append(f"(c) train_one_epoch, bs {a.batch} at {H}x{W}, seg_amd.AdamW, fused CE: ms per step over "
                 f"{a.loop_steps} steps, median (min..max) over {a.rounds} interleaved rounds")
    for k, t in ms.items():
        lines.append(f"    {k:58s} median {statistics.median(t):8.3f} ms   ({min(t):.3f}..{max(t):.3f})")
    k = list(ma)
    lines.append(f"(a) torch / seg_amd = {ma[k[1]] / ma[k[0]]:.2f}x per update call")
    k = list(mb)
    lines.append(f"(b) the update launch moves {12 * n / mb[k[0]] / 1e6:.2f} TB/s, one swap "
                 f"{16 * n / (mb[k[1]] / 2) / 1e6:.2f} TB/s (in-cache traffic)")
    d = statistics.median(ms["with ema=EMA(model)"]) - statistics.median(ms["without ema"])
    spread = max(max(t) - min(t) for t in ms.values())
    lines.append(f"(c) with - without = {1e3 * d:+.0f} us per step (difference of the medians; the larger of the two "
                 f"min..max spreads is {1e3 * spread:.0f} us)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
