"""Time the optimizer step and gradient clipping on one MI355X: seg_amd.AdamW / grad_norm beside torch's.

    python tools/optbench.py [--steps 200] [--rounds 5] [--parent DIR] [--out profiles/optim_bench.txt]

The tensors are MobileNetV2UNet(10)'s real parameter set with the gradients of one training step (the unused
classifier has none), copied once per optimizer so that every optimizer steps its own parameters and state.
  (a) seg_amd.AdamW.step() beside torch.optim.AdamW(foreach=True).step(), both on decay_groups(model, 1e-2)'s two
      groups; and the seg_adamw_step launches alone (the table already on the device);
  (b) grad_norm + step(grad_scale=...) beside torch.nn.utils.clip_grad_norm_ + the foreach step; and
      seg_amd.clip_grad_norm_ + torch's step (the path of an optimizer that is not ours);
  (c) seg_amd.Adam.step() of this tree beside the parent commit's (--parent: a checkout of it with its library built;
      its package is imported under another name and loads its own library), and the seg_adam_step_skip launch alone
      from either library, to show that the plain step did not move.
Each figure: `--steps` calls back to back between two device events (so a call that the host cannot issue as fast as
the device runs it is charged its host time), after a warm-up; the variants of a group alternate inside every one of
`--rounds` rounds; median and min..max over the rounds.  Needs an MI355X: there is no CPU path.
"""
import argparse
import importlib.util
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
from seg_amd.optim import _CHUNK, _chunk_map, _grad_table, _pack, _pack_w  # noqa: E402

DEV = "cuda"


def twin(model):
    """Another instance of the model (same modules, so decay_groups works) carrying the same gradients."""
    m = deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV).train()
    for p, q in zip(model.parameters(), m.parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    return m


def load_parent(path):
    """The parent checkout's seg_amd package under another name: its optim.py, its _lib.py, its own library."""
    pkg = os.path.join(path, "team02-objectdetection_amd", "seg_amd")
    spec = importlib.util.spec_from_file_location("seg_amd_parent", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["seg_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


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
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optbench.py needs an MI355X")
    model = deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV).train()
    x, y = synthetic_batch(2, 64, 64, 10, seed=111)
    model.forward_loss(x.to(DEV), y.to(DEV)).backward()
    torch.cuda.synchronize()
    live = [p for p in model.parameters() if p.grad is not None]
    n = sum(p.numel() for p in live)
    lines = [f"optimizer step and clipping, one MI355X: MobileNetV2UNet(10), {len(live)} tensors with a gradient, "
             f"{n} elements ({16 * n / 1e6:.0f} MB of p/g/m/v read + {12 * n / 1e6:.0f} MB written per step); us per "
             f"call, {a.steps} calls back to back between device events, median (min..max) over {a.rounds} "
             "interleaved rounds"]
    lr = 1e-3
    # (a) the step
    m1, m2 = twin(model), twin(model)
    ours = seg_amd.AdamW(decay_groups(m1, 1e-2), lr=lr)
    ref = torch.optim.AdamW(decay_groups(m2, 1e-2), lr=lr, foreach=True)
    ours.step()
    tables = []
    for g in ours.param_groups:  # the launches of one step, alone: the tables as the step packs them
        ps = [p for p in g["params"] if p.grad is not None]
        rows = [(p.data_ptr(), p.grad.data_ptr(), ours.state[p]["exp_avg"].data_ptr(),
                 ours.state[p]["exp_avg_sq"].data_ptr(), p.numel(), -lr, 1.0, 1 - lr * g["weight_decay"], 0.0)
                for p in ps]
        tables.append((_pack_w(rows).to(DEV), _chunk_map([p.numel() for p in ps], DEV)))
    stream = torch.cuda.current_stream().cuda_stream

    def launches():
        for t, cm in tables:
            call("seg_adamw_step", t.data_ptr(), cm.data_ptr(), cm.shape[0], _CHUNK, 0.1, 0.999, 0.001, 1e-8, None,
                 None, stream)

    la, ma = group("(a) AdamW step, two parameter groups (weights decayed, biases / BatchNorm not)",
                   {"seg_amd.AdamW.step()": ours.step, "torch.optim.AdamW(foreach=True).step()": ref.step,
                    "seg_adamw_step launches alone (2)": launches}, a.steps, a.rounds)
    lines += la
    # (b) clip + step
    m3 = twin(model)
    other = torch.optim.AdamW(decay_groups(m3, 1e-2), lr=lr, foreach=True)
    p1 = [p for g in ours.param_groups for p in g["params"]]
    p2 = [p for p in m2.parameters() if p.grad is not None]
    p3 = [p for p in m3.parameters() if p.grad is not None]
    max_norm = float(seg_amd.grad_norm(p1)[0]) * 10  # above the norm: the clip computes, the gradients stay

    def ours_clip():
        ours.step(grad_scale=seg_amd.grad_norm(p1, max_norm)[1:2])

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(p2, max_norm)
        ref.step()

    def mixed_clip():
        seg_amd.clip_grad_norm_(p3, max_norm)
        other.step()

    gt, gcm = _grad_table([p for p in p1 if p.grad is not None])
    work, out3 = torch.empty(gcm.shape[0], device=DEV), torch.empty(3, device=DEV)

    def sumsq_launches():
        call("seg_grad_sumsq", gt.data_ptr(), gcm.data_ptr(), gcm.shape[0], _CHUNK, max_norm, work.data_ptr(),
             out3.data_ptr(), stream)

    lb, mb = group("(b) global-norm clip + AdamW step (max_norm above the norm: no gradient changes)",
                   {"seg_amd.grad_norm + AdamW.step(grad_scale=...)": ours_clip,
                    "torch clip_grad_norm_ + foreach AdamW.step()": torch_clip,
                    "seg_amd.clip_grad_norm_ + foreach AdamW.step()": mixed_clip,
                    "seg_amd.grad_norm alone": lambda: seg_amd.grad_norm(p1, max_norm),
                    "seg_grad_sumsq launches alone (partials + finalize)": sumsq_launches}, a.steps, a.rounds)
    lines += lb
    # (c) the plain Adam step, this tree beside the parent commit
    m4 = twin(model)
    adam = seg_amd.Adam(m4.parameters(), lr=lr)
    adam.step()
    ps = [p for p in m4.parameters() if p.grad is not None]
    narrow = _pack([(p.data_ptr(), p.grad.data_ptr(), adam.state[p]["exp_avg"].data_ptr(),
                     adam.state[p]["exp_avg_sq"].data_ptr(), p.numel(), -lr, 1.0) for p in ps]).to(DEV)
    ncm = _chunk_map([p.numel() for p in ps], DEV)

    def plain_launch(fn):
        return lambda: fn("seg_adam_step_skip", narrow.data_ptr(), ncm.data_ptr(), ncm.shape[0], _CHUNK, 0.1, 0.999,
                          0.001, 1e-8, None, stream)

    fns = {"seg_amd.Adam.step(), this tree": adam.step,
           "seg_adam_step_skip launch alone, this tree's library": plain_launch(call)}
    if a.parent:
        parent = load_parent(a.parent)
        assert parent.optim.call is not call and not hasattr(parent, "AdamW")
        fns["seg_amd.Adam.step(), parent commit"] = parent.Adam(twin(model).parameters(), lr=lr).step
        fns["seg_adam_step_skip launch alone, parent's library"] = plain_launch(parent.optim.call)
    lc, _ = group("(c) plain seg_amd.Adam.step() (seg_adam_step_skip)" + ("" if a.parent else
                                                                           " -- parent commit not given: not measured"),
                  fns, a.steps, a.rounds)
    lines += lc
    k = list(ma)
    lines.append(f"(a) torch / seg_amd = {ma[k[1]] / ma[k[0]]:.2f}x per step() call; the launches alone move "
                 f"{28 * n / ma[k[2]] / 1e6:.2f} TB/s")
    k = list(mb)
    lines.append(f"(b) torch / seg_amd = {mb[k[1]] / mb[k[0]]:.2f}x per clip + step")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
