"""Time the temporal smoothing of Predictor on one MI355X: frames/s of the captured per-frame graph.

    python tools/temporalbench.py [--steps 1000] [--rounds 5] [--parent-tree DIR] [--out profiles/temporal_bench.txt]

The workload is the video loop's: MobileNetV2UNet(10), math="f16", a 720x1280 frame already on the device,
target_size (256, 128), graph replay (Predictor.step()).  Three predictors on the same model:
  plain              Predictor(model, math="f16")                               seg_argmax_nearest
  temporal           Predictor(model, math="f16", temporal=0.5)                 seg_temporal_argmax_nearest
  temporal+overlay   Predictor(model, math="f16", temporal=0.5, overlay=True)   ... + the overlay stage
Each figure: `--steps` replays back to back between two device events after a warm-up of 50 replays; the
three alternate inside every one of `--rounds` rounds; median and min..max over the rounds.

--parent-tree DIR names a built checkout of the parent commit.  The plain predictor is then also timed with
that tree's package and library, in processes of their own that alternate with processes timing this tree's
plain predictor the same way (`--only-plain --tree DIR`): the plain path is not touched by the smoothing, so
the two must agree within the run-to-run spread.  Needs an MI355X: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_HW, TARGET = (720, 1280), (256, 128)
WARMUP = 50


def use_tree(tree):
    for p in (os.path.join(tree, "team02-objectdetection_amd"), tree):
        sys.path.insert(0, p)


def timed(fn, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps  # us per frame


def measure(variants, steps, rounds):
    """{name: [us per frame, one per round]} of Predictor keyword sets, interleaved round by round."""
    import numpy as np
    import torch
    from seg_amd import MobileNetV2UNet, deterministic_init
    from seg_amd.infer import Predictor

    if not torch.cuda.is_available():
        raise SystemExit("temporalbench.py needs an MI355X")
    model = deterministic_init(MobileNetV2UNet(10), seed=11, random_running_stats=True).to("cuda").eval()
    g = np.random.Generator(np.random.PCG64(3))
    frame = torch.from_numpy(g.integers(0, 256, (*FRAME_HW, 3), dtype=np.uint8)).to("cuda")
    preds = {}
    for name, kw in variants.items():
        preds[name] = Predictor(model, frame_hw=FRAME_HW, target_size=TARGET, graph=True, math="f16", **kw)
        preds[name].set_frame(frame)
        for _ in range(WARMUP):
            preds[name].step()
    torch.cuda.synchronize()
    us = {k: [] for k in preds}
    for _ in range(rounds):
        for k, p in preds.items():
            us[k].append(timed(p.step, steps))
    return us


def line(name, t):
    med = statistics.median(t)
    return (f"    {name:44s} median {med:7.1f} us/frame = {1e6 / med:7.1f} frames/s   "
            f"({min(t):.1f}..{max(t):.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tree", default=REPO, help="checkout whose package and library are timed")
    ap.add_argument("--only-plain", action="store_true", help="time the plain predictor and print one JSON line")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.only_plain:
        use_tree(os.path.abspath(a.tree))
        print(json.dumps(measure({"plain": {}}, a.steps, a.rounds)["plain"]))
        return
    lines = [f"temporal smoothing of Predictor, one MI355X: MobileNetV2UNet(10), math f16, {FRAME_HW[0]}x{FRAME_HW[1]} "
             f"frame on the device -> {TARGET[0]}x{TARGET[1]}, graph replay; us per frame over {a.steps} replays "
             f"between device events after {WARMUP} warm-up replays, median (min..max) over {a.rounds} rounds"]
    if a.parent_tree:  # before this process opens the GPU: one child at a time
        runs = {"parent commit": [], "this tree": []}
        for _ in range(2):
            for name, tree in (("parent commit", os.path.abspath(a.parent_tree)), ("this tree", REPO)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-plain", "--tree", tree, "--steps",
                                    str(a.steps), "--rounds", str(a.rounds)], capture_output=True, text=True, cwd=tree)
                if r.returncode != 0:
                    raise SystemExit(f"timing the plain predictor of {tree} failed:\n{r.stdout}\n{r.stderr}")
                runs[name] += json.loads(r.stdout.strip().splitlines()[-1])
        lines.append("(a) the plain predictor, a process per tree, the trees alternating (2 processes each, rounds pooled)")
        lines += [line(f"plain, {k}", t) for k, t in runs.items()]
        d = statistics.median(runs["this tree"]) - statistics.median(runs["parent commit"])
        spread = max(max(t) - min(t) for t in runs.values())
        lines.append(f"    this tree - parent commit = {d:+.1f} us per frame (difference of the medians; the larger of the "
                     f"two min..max spreads is {spread:.1f} us)")
    use_tree(REPO)
    us = measure({"plain": {}, "temporal=0.5": {"temporal": 0.5},
                  "temporal=0.5, overlay=True": {"temporal": 0.5, "overlay": True}}, a.steps, a.rounds)
    lines.append("(b) this tree, one process, the three predictors alternating inside every round")
    lines += [line(k, t) for k, t in us.items()]
    med = {k: statistics.median(t) for k, t in us.items()}
    spread = max(max(t) - min(t) for t in us.values())
    lines.append(f"    temporal - plain = {med['temporal=0.5'] - med['plain']:+.1f} us per frame (the smoothed path has one "
                 f"launch more: update + labels-to-frame for the fused argmax); overlay on top: "
                 f"{med['temporal=0.5, overlay=True'] - med['temporal=0.5']:+.1f} us; the largest min..max spread is "
                 f"{spread:.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
