"""Time a distillation training step (seg_amd.DistillLoss) on one MI355X: fused against the unfused composition, and
beside the student's plain-CE step it is added to; then the seg_kd_* launches alone beside seg_cew_*.

    python tools/distillbench.py [--bs 32] [--hw 256 512] [--steps 10] [--rounds 3] [--out profiles/distill_bench.txt]

Student MobileNetV2UNet(10) in train(), teacher UNet(10) in eval (the same conv math as the student), one
device-resident batch of a synthetic road scene, seg_amd.Adam, at conv math f32 and bf16io:
  (a) the student alone with plain nn.CrossEntropyLoss, fused (what distillation is added to);
  (b) DistillLoss(teacher) fused: compute_loss -> teacher.forward_low_logits, student.forward_loss (seg_kd_*);
  (c) the same criterion unfused: criterion(model(x), t, criterion.teacher_logits(x)) -- both models' full-resolution
      NCHW fp32 logits, the two log-softmaxes and the KL in torch ops, autograd's temporaries.
A step is train_one_epoch's inner step: zero_grad, the loss, backward, _step_and_loss (the optimizer step and
loss.item()).  Each figure: `--steps` steps between two device events, after a warm-up that records the tapes; the
variants alternate inside every one of `--rounds` rounds; median and min..max over the rounds.  Peak memory is
torch.cuda.max_memory_allocated over a variant's timed steps (every variant's plans stay resident, so the differences
are what a step allocates on top).

The kernels alone: seg_kd_upsample_loss / _grad beside seg_cew_upsample_loss / _grad on the same student rows and
labels (fp32, class weights on), the teacher at the student's low resolution and at the output resolution; us per
launch over `--launches` launches between two device events, and the bytes each must move (student rows, teacher
rows, labels; the gradient rows written).  Not measured here: more than one GPU, and convergence of a full run.
Needs an MI355X: there is no CPU path.
"""
import argparse
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
from seg_amd._lib import call, query  # noqa: E402
from seg_amd.detinit import synthetic_scene  # noqa: E402

DEV = "cuda"
C = 10


def stepper(conv_math, loss_of, x, y):
    """One variant: its own student and optimizer; loss_of(model) -> the step's loss."""
    model = seg_amd.deterministic_init(seg_amd.MobileNetV2UNet(C), seed=11).to(DEV).train()
    engine.set_conv_math(model, conv_math)
    opt = seg_amd.Adam(model.parameters(), lr=1.5e-4)

    def step():
        opt.zero_grad()
        loss = loss_of(model)
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


def launches(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def kernels_alone(bs, H, W, n, lines):
    """seg_kd_* beside seg_cew_* on one set of student rows [bs, H/2, W/2, 12] and labels [bs, H, W]."""
    s = torch.cuda.current_stream().cuda_stream
    Hl, Wl, ld = H // 2, W // 2, (C + 3) & ~3
    g = torch.Generator().manual_seed(5)
    low = (torch.randn(bs * Hl * Wl, ld, generator=g) * 2).to(DEV)
    y = torch.randint(0, C, (bs, H, W), generator=g)
    y[:, :8] = -100
    y = y.to(DEV)
    w = (torch.rand(C, generator=g) * 3 + 0.05).to(DEV)
    pixels = bs * H * W
    dhigh = torch.empty(pixels * ld, device=DEV)
    gout = torch.ones(1, device=DEV)
    st4, st6 = torch.zeros(4, device=DEV), torch.zeros(6, device=DEV)
    wc = torch.empty(query("seg_cew_workspace_floats", pixels), device=DEV)
    wk = torch.empty(query("seg_kd_workspace_floats", pixels), device=DEV)
    base = (low.data_ptr(), ld, bs, Hl, Wl, C)
    lab = (y.data_ptr(), H, W, -100, w.data_ptr())
    rows_b, lab_b, grad_b = low.numel() * 4, pixels * 8, dhigh.numel() * 4
    mib = lambda b: f"{b / 2**20:.0f} MiB"  # noqa: E731
    lines.append(f"kernels alone, fp32, bs {bs}, student rows {Hl}x{Wl}x{ld} -> {H}x{W}, class weights on, labels "
                 f"int64 (the first 8 rows of every image ignored); us per launch over {n} launches")
    t = launches(lambda: call("seg_cew_upsample_loss", *base, *lab, 0.0, 0, wc.data_ptr(), st4.data_ptr(), s), n)
    lines.append(f"  seg_cew_upsample_loss                       {t:8.1f} us   moves {mib(rows_b + lab_b)} "
                 f"(rows {mib(rows_b)} + labels {mib(lab_b)})")
    t = launches(lambda: call("seg_cew_upsample_grad", *base, *lab, 0.0, gout.data_ptr(), st4.data_ptr(),
                              dhigh.data_ptr(), ld, s), n)
    lines.append(f"  seg_cew_upsample_grad                       {t:8.1f} us   moves {mib(rows_b + lab_b + grad_b)} "
                 f"(+ gradient rows {mib(grad_b)})")
    for Ht, Wt in ((Hl, Wl), (H, W)):
        te = (torch.randn(bs * Ht * Wt, ld, generator=g) * 2).to(DEV)
        te_b = te.numel() * 4
        kd = (te.data_ptr(), ld, Ht, Wt)
        opt = (1.0, 1.0, 2.0, 1)
        t = launches(lambda: call("seg_kd_upsample_loss", *base, *kd, *lab, *opt, wk.data_ptr(), st6.data_ptr(), s), n)
        lines.append(f"  seg_kd_upsample_loss, teacher {Ht:4d}x{Wt:<4d}     {t:8.1f} us   moves "
                     f"{mib(rows_b + te_b + lab_b)} (+ teacher rows {mib(te_b)})")
        t = launches(lambda: call("seg_kd_upsample_grad", *base, *kd, *lab, *opt, gout.data_ptr(), st6.data_ptr(),
                                  dhigh.data_ptr(), ld, s), n)
        lines.append(f"  seg_kd_upsample_grad, teacher {Ht:4d}x{Wt:<4d}     {t:8.1f} us   moves "
                     f"{mib(rows_b + te_b + lab_b + grad_b)}")
        del te


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--hw", type=int, nargs=2, default=(256, 512))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distillbench.py needs an MI355X")
    H, W = a.hw
    x, y = (t.to(DEV) for t in synthetic_scene(a.bs, H, W, C, seed=100))
    plain = nn.CrossEntropyLoss()
    pixels = a.bs * H * W
    lines = [f"distillation training step, one MI355X: student MobileNetV2UNet({C}) train(), teacher UNet({C}) eval "
             f"(the student's conv math), one resident batch {a.bs}x3x{H}x{W} ({pixels} pixels), seg_amd.Adam; ms per "
             f"step (zero_grad, loss, backward, optimizer step, loss.item()), {a.steps} steps between device events, "
             f"median (min..max) over {a.rounds} interleaved rounds; peak = torch.cuda.max_memory_allocated over the "
             "timed steps",
             "(a) student alone, plain nn.CrossEntropyLoss fused, (b) DistillLoss(teacher, 1, 1, T=2) fused, (c) the "
             "same criterion unfused: full-resolution logits of both models, torch forward"]
    for conv_math in ("f32", "bf16io"):
        teacher = seg_amd.deterministic_init(seg_amd.UNet(C), seed=12).to(DEV)
        engine.set_conv_math(teacher, conv_math)
        crit = seg_amd.DistillLoss(teacher, 1.0, 1.0, 2.0).to(DEV)
        variants = {"a plain CE fused": stepper(conv_math, lambda m: train.compute_loss(m, plain, x, y), x, y),
                    "b distill fused": stepper(conv_math, lambda m: train.compute_loss(m, crit, x, y), x, y),
                    "c distill unfused": stepper(conv_math, lambda m: crit(m(x), y, crit.teacher_logits(x)), x, y)}
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
            lines.append(f"{conv_math:7s}{k:20s} median {med[k]:7.2f} ms  ({min(ms[k]):.2f}..{max(ms[k]):.2f})   "
                         f"peak {peak[k] / 2**20:8.0f} MiB   last loss {loss[k]:.4f}")
        b, c = "b distill fused", "c distill unfused"
        lines.append(f"{conv_math:7s}unfused / fused = {med[c] / med[b]:.3f}x step time ({med[c] - med[b]:+.2f} ms), "
                     f"{(peak[c] - peak[b]) / 2**20:.0f} MiB more at peak (one model's N*C*Ho*Wo*4 = "
                     f"{a.bs * C * H * W * 4 / 2**20:.0f} MiB); distill fused - plain CE fused = "
                     f"{med[b] - med['a plain CE fused']:+.2f} ms per step (the teacher's forward and the second "
                     f"tensor in the loss kernels); the largest min..max spread is "
                     f"{1e3 * max(max(v) - min(v) for v in ms.values()):.0f} us")
        for _, release in variants.values():
            release()
        engine.release_plans(teacher)
        del variants, teacher, crit
        torch.cuda.empty_cache()
    kernels_alone(a.bs, H, W, a.launches, lines)
    lines.append("not measured: more than one GPU, convergence of a full distillation run")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
