"""GPU: the SGD / poly recipe through the training loop -- MobileNetV2UNet(10) at 2x3x64x64,
seg_amd.SGD(decay_groups(model, 5e-4), lr=1e-2, momentum=0.9, nesterov=True), seg_amd.PolyLR and
train_one_epoch(..., max_grad_norm=, scheduler=).

The reference of a step is torch's: a twin list of cloned parameters in the same two groups, stepped by
torch.optim.SGD(foreach=True) under a PolyLR of its own.  After each of our steps the twin receives OUR model's
.grad (which the loop leaves unclipped and unwritten), clips it with torch.nn.utils.clip_grad_norm_ to the same
maximum and steps: the optimizer is compared on the same gradients, three steps long, without the divergence that a
second model's own gradients would bring from the second step on.  Parameters agree to rtol 2e-5 (the clip
coefficient's 1e-5 plus rounding; tests/test_gpu_adamw_model.py) and atol 1e-7.
"""
import pytest
import torch
from torch import nn

import seg_amd
from seg_amd import SGD, AdamW, MobileNetV2UNet, PolyLR, decay_groups, freeze, grad_norm, train_model, train_one_epoch
from seg_amd.detinit import deterministic_init, synthetic_batch
from seg_amd.train import compute_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 1e-2, 5e-4


def build():
    return deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV).train()


def recipe(model, total_iters=3):
    opt = SGD(decay_groups(model, WD), lr=LR, momentum=0.9, nesterov=True)
    return opt, PolyLR(opt, total_iters=total_iters, warmup_iters=1)


@pytest.fixture(scope="module")
def batch():
    return synthetic_batch(2, 64, 64, 10, seed=111)


@pytest.fixture(scope="module")
def max_norm(batch):
    """Half the measured gradient norm of the first step: the clip is active."""
    x, y = batch
    model = build()
    compute_loss(model, nn.CrossEntropyLoss(), x.to(DEV), y.to(DEV)).backward()
    return float(grad_norm(list(model.parameters()))[0]) / 2


def one(model, opt, xy, max_norm, **kw):
    return train_one_epoch(model, [xy], nn.CrossEntropyLoss(), opt, DEV, progress=False, max_grad_norm=max_norm, **kw)


def buffers_of(opt):
    return [opt.state[p]["momentum_buffer"] if "momentum_buffer" in opt.state.get(p, {}) else None
            for g in opt.param_groups for p in g["params"]]


def test_three_steps_match_torch(batch, max_norm):
    ours, again = build(), build()
    start = {k: p.detach().clone() for k, p in ours.named_parameters()}
    opt, sched = recipe(ours)
    groups = [{"params": [torch.nn.Parameter(p.detach().clone()) for p in g["params"]],
               "weight_decay": g["weight_decay"]} for g in opt.param_groups]
    pairs = [(p, q) for g, h in zip(opt.param_groups, groups) for p, q in zip(g["params"], h["params"])]
    ref = torch.optim.SGD(groups, lr=LR, momentum=0.9, nesterov=True, foreach=True)
    ref_sched = PolyLR(ref, total_iters=3, warmup_iters=1)
    lrs, ref_lrs = [], []
    for step in range(3):
        lrs.append([g["lr"] for g in opt.param_groups])
        ref_lrs.append([g["lr"] for g in ref.param_groups])
        one(ours, opt, batch, max_norm, scheduler=sched)
        for p, q in pairs:
            q.grad = None if p.grad is None else p.grad.clone()
        live = [q for _, q in pairs if q.grad is not None]
        norm = float(torch.nn.utils.clip_grad_norm_(live, max_norm))
        ref.step()
        ref_sched.step()
        torch.cuda.synchronize()
        coef = float(grad_norm([p for p, _ in pairs], max_norm)[1])
        print(f"step {step}: lr {lrs[-1]}, norm {norm:.6g}, coefficient {coef:.6g}")
        assert (0.49 < coef < 0.51) if step == 0 else coef <= 1.0
        for i, (p, q) in enumerate(pairs):
            torch.testing.assert_close(p, q, rtol=2e-5, atol=1e-7, msg=lambda m: f"step {step}, parameter {i}: {m}")
    assert lrs == ref_lrs and sched.last_epoch == ref_sched.last_epoch == 3
    assert lrs[0] == [LR * 0.1] * 2 and lrs[1][0] == pytest.approx(LR * (2 / 3) ** 0.9, rel=1e-12)
    assert [g["lr"] for g in opt.param_groups] == [0.0, 0.0]  # t = total_iters
    with_grad = [k for k, p in ours.named_parameters() if p.grad is not None]
    moved = sum(int(not torch.equal(p, start[k])) for k, p in ours.named_parameters())
    assert moved > len(with_grad) // 2
    for p, q in pairs:  # the state is torch's: one buffer per parameter that had a gradient
        assert list(opt.state.get(p, {})) == list(ref.state.get(q, {})) == (["momentum_buffer"] if p.grad is not None
                                                                            else [])
    # a second model trained the same way: bitwise, BatchNorm statistics included
    opt2, sched2 = recipe(again)
    for step in range(3):
        one(again, opt2, batch, max_norm, scheduler=sched2)
    torch.cuda.synchronize()
    for (k, a), b in zip(ours.state_dict().items(), again.state_dict().values()):
        assert torch.equal(a, b), k
    assert any(k.endswith("running_mean") for k in ours.state_dict())


def test_frozen_backbone(batch, max_norm):
    model = build()
    opt, sched = recipe(model)  # over every parameter, built before the backbone is frozen
    freeze(model)
    model.train()
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    for _ in range(2):
        one(model, opt, batch, max_norm, scheduler=sched)
    torch.cuda.synchronize()
    moved = 0
    for k, p in model.named_parameters():
        if k.startswith("backbone."):
            assert p.grad is None and torch.equal(p, start[k]), k  # bitwise where it was
            assert p not in opt.state or len(opt.state[p]) == 0, k
        else:
            moved += int(not torch.equal(p, start[k]))
    assert moved > 0 and len(opt.state_dict()["state"]) == sum(b is not None for b in buffers_of(opt)) > 0


@pytest.mark.parametrize("with_ema", [False, True])
def test_out_of_range_label_skips_the_step(batch, max_norm, with_ema):
    x, y = batch
    bad = y.clone()
    bad[0, 0, 0] = 10
    model = build()
    opt, sched = recipe(model, total_iters=10)
    ema = seg_amd.EMA(model, 0.9) if with_ema else None
    kw = {"scheduler": sched, "ema": ema}
    one(model, opt, (x, y), max_norm, **kw)
    torch.cuda.synchronize()
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    bufs = [None if b is None else b.clone() for b in buffers_of(opt)]
    shadows = [e.clone() for e in ema.shadows] if with_ema else None
    lr = [g["lr"] for g in opt.param_groups]
    with pytest.raises(IndexError):
        one(model, opt, (x, bad), max_norm, **kw)
    torch.cuda.synchronize()
    assert sched.last_epoch == 1 and [g["lr"] for g in opt.param_groups] == lr  # the scheduler was not touched
    for k, p in model.named_parameters():
        assert torch.equal(p, params[k]), k
    now = buffers_of(opt)
    assert [b is None for b in now] == [b is None for b in bufs] and any(b is not None for b in bufs)
    assert all(torch.equal(a, b) for a, b in zip(now, bufs) if a is not None)
    if with_ema:  # the skipped batch leaves the average where it was; a good batch moves it
        assert ema.num_updates == 1 and all(torch.equal(a, b) for a, b in zip(ema.shadows, shadows))
    one(model, opt, (x, y), max_norm, **kw)
    torch.cuda.synchronize()
    assert sched.last_epoch == 2
    assert any(not torch.equal(p, params[k]) for k, p in model.named_parameters())
    if with_ema:
        assert ema.num_updates == 2 and any(not torch.equal(a, b) for a, b in zip(ema.shadows, shadows))


def test_out_of_range_label_in_the_very_first_batch(batch, max_norm):
    x, y = batch
    bad = y.clone()
    bad[0, 0, 0] = 10
    model, fresh = build(), build()
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt, sched = recipe(model)
    empty = opt.state_dict()
    with pytest.raises(IndexError):
        one(model, opt, (x, bad), max_norm, scheduler=sched)
    torch.cuda.synchronize()
    assert sched.last_epoch == 0
    assert opt.state_dict()["state"] == {} == empty["state"]  # no momentum_buffer entries are left behind
    for k, p in model.named_parameters():
        assert torch.equal(p, start[k]), k
    one(model, opt, (x, y), max_norm, scheduler=sched)  # torch's first step: the buffers are seeded with d
    opt2, sched2 = recipe(fresh)
    one(fresh, opt2, (x, y), max_norm, scheduler=sched2)
    torch.cuda.synchronize()
    for (k, p), q in zip(model.named_parameters(), fresh.parameters()):
        assert torch.equal(p, q), k
    for a, b in zip(buffers_of(opt), buffers_of(opt2)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert sched.last_epoch == sched2.last_epoch == 1


def test_train_model_without_scheduler_is_unchanged(batch):
    x, y = batch
    x2, y2 = synthetic_batch(2, 64, 64, 10, seed=112)
    a, b = build(), build()
    oa, ob = AdamW(decay_groups(a, 1e-2), lr=1e-3), AdamW(decay_groups(b, 1e-2), lr=1e-3)
    kw = dict(epochs=1, checkpoint_pattern=None, progress=False)
    train_model(a, [(x, y), (x2, y2)], nn.CrossEntropyLoss(), oa, DEV, scheduler=None, **kw)
    train_model(b, [(x, y), (x2, y2)], nn.CrossEntropyLoss(), ob, DEV, **kw)
    for (k, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(p, q), k
