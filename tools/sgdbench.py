"""Time the SGD step on one MI355X: seg_amd.SGD beside torch's foreach SGD and beside our own Adam launch.

    python tools/sgdbench.py [--steps 200] [--rounds 5] [--out profiles/sgd_bench.txt]

The tensors are MobileNetV2UNet(10)'s real parameter set with the gradients of one training step (the unused
classifier has none), copied once per optimizer so that every optimizer steps its own parameters and state.  The
recipe is the road-scene one: decay_groups(model, 5e-4)'s two groups, lr 1e-2, momentum 0.9, Nesterov.
  (a) seg_amd.SGD.step() beside torch.optim.SGD(foreach=True).step() on the same groups;
  (b) the launches alone, the tables already on the device: the two seg_sgd_step launches of (a)'s step, the same
      two with momentum 0 (three streams: no buffer), and, from the same library over the same tensors, one
      seg_adam_step_skip launch (seven streams to SGD's five) -- the comparison point for the device side.
Each figure: `--steps` calls back to back between two device events (so a call that the host cannot issue as fast as
the device runs it is charged its host time), after a warm-up; the variants of a group alternate inside every one of
`--rounds` rounds; median and min..max over the rounds.  Needs an MI355X: there is no CPU path.
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "team02-objectdetection_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import seg_amd  # noqa: E402
from seg_amd import MobileNetV2UNet, decay_groups, deterministic_init, synthetic_batch  # noqa: E402
from seg_amd._lib import call  # noqa: E402
from seg_amd.optim import _CHUNK, _chunk_map, _pack, _pack_w  # noqa: E402

DEV = "cuda"
LR, WD, MOMENTUM = 1e-2, 5e-4, 0.9


def twin(model):
    """Another instance of the model (same modules, so decay_groups works) carrying the same gradients."""
    m = deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV).train()
    for p, q in zip(model.parameters(), m.parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    return m


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps


def group(title, fns, steps, rounds):
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
        lines.append(f"    {k:58s} median {statistics.median(t):8.1f} us   ({min(t):.1f}..{max(t):.1f})")
    return lines, {k: statistics.median(t) for k, t in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgdbench.py needs an MI355X")
    model = deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV).train()
    x, y = synthetic_batch(2, 64, 64, 10, seed=111)
    model.forward_loss(x.to(DEV), y.to(DEV)).backward()
    torch.cuda.synchronize()
    live = [p for p in model.parameters() if p.grad is not None]
    n = sum(p.numel() for p in live)
    lines = [f"SGD step (momentum {MOMENTUM}, Nesterov, weight decay {WD} on the weights), one MI355X: "
             f"MobileNetV2UNet(10), {len(live)} tensors with a gradient, {n} elements ({12 * n / 1e6:.0f} MB of "
             f"p / g / buf read + {8 * n / 1e6:.0f} MB written per step); us per call, {a.steps} calls back to back "
             f"between device events, median (min..max) over {a.rounds} interleaved rounds"]
    # (a) the step
    m1, m2 = twin(model), twin(model)
    ours = seg_amd.SGD(decay_groups(m1, WD), lr=LR, momentum=MOMENTUM, nesterov=True)
    ref = torch.optim.SGD(decay_groups(m2, WD), lr=LR, momentum=MOMENTUM, nesterov=True, foreach=True)
    ours.step()
    ref.step()
    la, ma = group("(a) SGD step, two parameter groups (weights decayed, biases / BatchNorm not)",
                   {"seg_amd.SGD.step()": ours.step, "torch.optim.SGD(foreach=True).step()": ref.step},
                   a.steps, a.rounds)
    lines += la
    # (b) the launches alone
    tables = []
    for g in ours.param_groups:  # the tables as a step after the first packs them: seed flag 0
        ps = [p for p in g["params"] if p.grad is not None]
        rows = [(p.data_ptr(), p.grad.data_ptr(), ours.state[p]["momentum_buffer"].data_ptr(), 0, p.numel(),
                 0.0, 1.0, 1.0, 0.0) for p in ps]
        tables.append((_pack_w(rows).to(DEV), _chunk_map([p.numel() for p in ps], DEV), g["weight_decay"]))
    stream = torch.cuda.current_stream().cuda_stream

    def sgd_launches(momentum, nesterov):
        def fn():
            for t, cm, wd in tables:
                call("seg_sgd_step", t.data_ptr(), cm.data_ptr(), cm.shape[0], _CHUNK, LR, momentum, 1.0, wd, nesterov,
                     None, None, stream)
        return fn

    m3 = twin(model)
    adam = seg_amd.Adam(m3.parameters(), lr=1e-3)
    adam.step()
    ps = [p for p in m3.parameters() if p.grad is not None]
    narrow = _pack([(p.data_ptr(), p.grad.data_ptr(), adam.state[p]["exp_avg"].data_ptr(),
                     adam.state[p]["exp_avg_sq"].data_ptr(), p.numel(), -1e-3, 1.0) for p in ps]).to(DEV)
    ncm = _chunk_map([p.numel() for p in ps], DEV)

    def adam_launch():
        call("seg_adam_step_skip", narrow.data_ptr(), ncm.data_ptr(), ncm.shape[0], _CHUNK, 0.1, 0.999, 0.001, 1e-8,
             None, stream)

    lb, mb = group("(b) the launches alone (tables on the device), same library, same tensors",
                   {"seg_sgd_step launches (2): momentum, Nesterov, decay": sgd_launches(MOMENTUM, 1),
                    "seg_sgd_step launches (2): momentum 0 (no buffer)": sgd_launches(0.0, 0),
                    "seg_adam_step_skip launch (1): p, g, m, v": adam_launch}, a.steps, a.rounds)
    lines += lb
    k = list(ma)
    lines.append(f"(a) torch / seg_amd = {ma[k[1]] / ma[k[0]]:.2f}x per step() call")
    k = list(mb)
    lines.append(f"(b) the SGD launches move {20 * n / mb[k[0]] / 1e6:.2f} TB/s (5 streams), without momentum "
                 f"{12 * n / mb[k[1]] / 1e6:.2f} TB/s (3 streams), the Adam launch {28 * n / mb[k[2]] / 1e6:.2f} TB/s "
                 f"(7 streams); SGD / Adam = {mb[k[0]] / mb[k[2]]:.2f}x in time")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
