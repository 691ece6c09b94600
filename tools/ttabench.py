"""Time test-time augmentation on one MI355X.

    python tools/ttabench.py [--rounds 5] [--out profiles/tta_bench.txt]

(a) The ensemble step: seg_tta_upsample_eval on given low-resolution logits against the torch composition of the
    same step -- per view upsample (align_corners=True), flip, softmax, weighted sum; then argmax, bincount of
    label * C + class over the valid pixels, NLL of log p -- in the same process, the two alternating inside
    every round.  2 views (a flip pair) and 6 views (scales 0.75 / 1 / 1.25 with their flips) at the
    MobileNetV2UNet shape (256x512, batch 32: logits at half resolution) and the UNet shape (512x1024, batch 8:
    logits at full resolution), 10 classes.  The one fixed condition: the fused step is not slower.
(b) Validation per batch: model.forward_metrics against forward_metrics_tta with "hflip" and TTA((0.75, 1, 1.25)),
    MobileNetV2UNet(10), 256x512, batch 32 -- the views' forwards included.
(c) Predictor frames/s (720x1280 frame on the device -> 256x128, graph replay): plain, "hflip" as one batch-2
    forward and as two batch-1 forwards with math f32, and plain against "hflip" (two batch-1 forwards, its
    default there) with math f16.
Every figure: back-to-back calls between two device events after a warm-up, median (min..max) over the rounds.
(b) and (c) are recorded, not gated.  Needs an MI355X: there is no CPU path.
"""
import argparse
import ctypes
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "team02-objectdetection_amd"), REPO):
    sys.path.insert(0, _p)

C = 10


def timed(fn, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps  # us per call


def alternate(fns, steps, rounds, warmup):
    us = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    for _ in range(rounds):
        for k, fn in fns.items():
            us[k].append(timed(fn, steps))
    return us


def line(name, t, unit="us"):
    return f"    {name:52s} median {statistics.median(t):9.1f} {unit}   ({min(t):.1f}..{max(t):.1f})"


def ensemble_step(N, Ho, Wo, low_hws, rounds):
    """(fused us, torch us) per call for views of the given low-resolution sizes, each plain and mirrored."""
    import torch
    import torch.nn.functional as F
    from seg_amd._lib import call, query
    from seg_amd.tta import view_table
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    ld = (C + 3) // 4 * 4
    lows, flips = [], []
    for H, W in low_hws:
        for flip in (False, True):
            lo = torch.zeros((N, H, W, ld), device=dev)
            lo[..., :C] = 3.0 * torch.randn((N, H, W, C), device=dev, generator=g)
            lows.append(lo)
            flips.append(flip)
    w = [1.0 / len(lows)] * len(lows)
    y = torch.randint(0, C, (N, Ho, Wo), device=dev, generator=g)
    y[torch.rand((N, Ho, Wo), device=dev, generator=g) < 0.1] = -100
    views = view_table(lows, flips, w)
    work = torch.empty(query("seg_tta_workspace_floats", N * Ho * Wo), device=dev)
    out4 = torch.empty(4, device=dev)
    conf = torch.zeros((C, C), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def fused():
        call("seg_tta_upsample_eval", ctypes.addressof(views), len(lows), N, C, y.data_ptr(), Ho, Wo, -100, None, 0,
             work.data_ptr(), out4.data_ptr(), conf.data_ptr(), None, s)

    conf_t = torch.zeros((C, C), dtype=torch.int64, device=dev)
    res = {}

    def composed():
        p = None
        for lo, flip, wk in zip(lows, flips, w):
            z = lo[..., :C].permute(0, 3, 1, 2)
            if (z.shape[2], z.shape[3]) != (Ho, Wo):
                z = F.interpolate(z, (Ho, Wo), mode="bilinear", align_corners=True)
            if flip:
                z = torch.flip(z, (-1,))
            t = torch.softmax(z, 1) * wk
            p = t if p is None else p + t
        keep = y != -100
        conf_t.add_(torch.bincount(y[keep] * C + p.argmax(1)[keep], minlength=C * C).view(C, C))
        res["loss"] = F.nll_loss(torch.log(p), y, ignore_index=-100)

    us = alternate({"fused": fused, "torch": composed}, 20, rounds, 3)
    # the two compute the same thing
    conf.zero_()
    conf_t.zero_()
    fused()
    composed()
    torch.cuda.synchronize()
    agree = float((conf == conf_t).float().mean())
    rel = abs(out4[0].item() - res["loss"].item()) / abs(res["loss"].item())
    return us, agree, rel


def validation(rounds):
    import torch
    from seg_amd import MobileNetV2UNet, TTA, deterministic_init
    model = deterministic_init(MobileNetV2UNet(C), seed=7, random_running_stats=True).to("cuda").eval()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(32, 3, 256, 512, generator=g).to("cuda")
    y = torch.randint(0, C, (32, 256, 512), generator=g).to("cuda")
    conf = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    scales = TTA((0.75, 1, 1.25))
    fns = {"plain: forward_metrics": lambda: model.forward_metrics(x, y, conf),
           'tta "hflip" (2 views)': lambda: model.forward_metrics_tta(x, y, conf, "hflip"),
           "tta TTA((0.75, 1, 1.25)) (6 views)": lambda: model.forward_metrics_tta(x, y, conf, scales)}
    return alternate(fns, 5, rounds, 2)


def predictors(rounds):
    import numpy as np
    import torch
    from seg_amd import MobileNetV2UNet, deterministic_init
    from seg_amd.infer import Predictor
    model = deterministic_init(MobileNetV2UNet(C), seed=11, random_running_stats=True).to("cuda").eval()
    frame = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).integers(0, 256, (720, 1280, 3),
                                                                             dtype=np.uint8)).to("cuda")
    variants = {"f32 plain": dict(math="f32"),
                'f32 "hflip", one batch-2 forward': dict(math="f32", tta="hflip", tta_batch=True),
                'f32 "hflip", two batch-1 forwards': dict(math="f32", tta="hflip", tta_batch=False),
                "f16 plain": dict(math="f16"),
                'f16 "hflip", two batch-1 forwards': dict(math="f16", tta="hflip")}
    fns = {}
    for name, kw in variants.items():
        p = Predictor(model, frame_hw=(720, 1280), target_size=(256, 128), graph=True, **kw)
        p.set_frame(frame)
        fns[name] = p.step
    return alternate(fns, 300, rounds, 50)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ttabench.py needs an MI355X")
    lines = [f"test-time augmentation, one MI355X; median (min..max) over {a.rounds} rounds of back-to-back calls between "
             "two device events after a warm-up, the variants of a group alternating inside every round",
             f"(a) the ensemble step on given low-resolution logits, {C} classes, us per call (20 calls per round): "
             "seg_tta_upsample_eval against the torch composition (upsample, flip, softmax, weighted sum, argmax, "
             "bincount, NLL)"]
    met = True
    shapes = {"256x512 bs 32 (logits at 1/2)": (32, 256, 512, 2), "UNet 512x1024 bs 8 (logits at 1/1)": (8, 512, 1024, 1)}
    for name, (N, Ho, Wo, div) in shapes.items():
        for label, scales in (("2 views", (1.0,)), ("6 views", (0.75, 1.0, 1.25))):
            hws = [(int(Ho * s) // div, int(Wo * s) // div) for s in scales]
            us, agree, rel = ensemble_step(N, Ho, Wo, hws, a.rounds)
            f, t = statistics.median(us["fused"]), statistics.median(us["torch"])
            met = met and f <= t
            lines += [line(f"{name}, {label}: fused", us["fused"]), line(f"{name}, {label}: torch", us["torch"]),
                      f"        torch / fused = {t / f:.1f}x; matrices agree in {100 * agree:.2f} % of their bins, "
                      f"losses to {rel:.1e} relative"]
            torch.cuda.empty_cache()
    lines.append(f"    condition (a), the fused step is not slower than the torch composition: {'met' if met else 'NOT met'}")
    lines.append("(b) validation per batch, MobileNetV2UNet(10) f32, 256x512, batch 32, us per batch (5 per round), the "
                 "views' forwards included")
    lines += [line(k, t) for k, t in validation(a.rounds).items()]
    torch.cuda.empty_cache()
    lines.append("(c) Predictor, MobileNetV2UNet(10), 720x1280 frame on the device -> 256x128, graph replay, us per frame "
                 "(300 per round)")
    for k, t in predictors(a.rounds).items():
        lines.append(line(k, t) + f"   = {1e6 / statistics.median(t):7.1f} frames/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if not met:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
