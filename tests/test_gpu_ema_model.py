"""GPU: seg_amd.EMA on the real models through the training loop -- UNet(4) at 2x3x32x64 and MobileNetV2UNet(10) at
2x3x64x64, deterministic_init and synthetic_batch, seg_amd.AdamW.

The shadows are checked against the float64 recurrence over snapshots of the live state_dict (the bound of
tests/test_gpu_ema.py: k * 2^-21 * M after k updates).  Everything about the exchange is checked bitwise: the engine's
reductions are fixed-order and a model loaded with the averaged state_dict picks the same routes, so evaluation under
applied() must equal evaluation of that model bit for bit -- any difference is a stale derived weight -- and a run
that swapped in between must equal a twin that never did.
"""
import os
import socket

import pytest
import torch
from torch import nn

from seg_amd import (AdamW, EMA, MobileNetV2UNet, Predictor, UNet, decay_groups, engine, freeze, train_one_epoch,
                     validate)
from seg_amd.detinit import deterministic_init, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 1e-3
DECAY = 0.9
ARCHS = {"unet": (lambda: UNet(4), 4, (32, 64)), "mnv2": (lambda: MobileNetV2UNet(10), 10, (64, 64))}


def build(arch, seed=11, math=None):
    m = deterministic_init(ARCHS[arch][0](), seed=seed).to(DEV).train()
    if math is not None:
        engine.set_conv_math(m, math)
    return m


def batches(arch, n, seed0=111):
    _, C, (H, W) = ARCHS[arch]
    return [synthetic_batch(2, H, W, C, seed=seed0 + i) for i in range(n)]


def optimizer(model):
    return AdamW(decay_groups(model, 1e-2), lr=LR)


def snapshot(model):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in getattr(model, "module", model).state_dict().items()}


def trained(arch, steps=3, math=None, seed0=111):
    """A model, its EMA and optimizer after `steps` one-batch epochs, and the state_dict snapshots after each."""
    model = build(arch, math=math)
    ema, opt = EMA(model, decay=DECAY), optimizer(model)
    snaps = [snapshot(model)]
    for b in batches(arch, steps, seed0):
        train_one_epoch(model, [b], nn.CrossEntropyLoss(), opt, DEV, progress=False, ema=ema)
        snaps.append(snapshot(model))
    return model, ema, opt, snaps


def fresh_with(arch, sd, math=None):
    m = build(arch, seed=99, math=math)
    m.load_state_dict(sd, strict=True)
    return m


def same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("arch", list(ARCHS))
def test_shadows_after_three_steps(arch):
    model, ema, opt, snaps = trained(arch, 3)
    assert ema.num_updates == 3
    w = float(torch.tensor(1.0 - DECAY, dtype=torch.float32))
    worst, moved = 0.0, 0
    for k in ema.names:
        e64 = snaps[0][k].double().clone()
        M = e64.abs()
        for s in snaps[1:]:
            p = s[k].double()
            e64 += w * (p - e64)
            M = torch.maximum(M, torch.maximum(p.abs(), e64.abs()))
        e = ema.shadows[ema._slot[k]]
        err = (e.double() - e64).abs()
        bound = 3 * 2.0 ** -21 * M
        assert bool((err <= bound).all()), (k, float(err.max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        moved += int(not torch.equal(e, snaps[0][k]))
    print(f"{arch}: worst error / bound {worst:.3f}; {moved} of {len(ema.names)} shadows moved")
    assert moved > len(ema.names) // 2
    avg = ema.averaged_state_dict()
    assert list(avg) == list(snaps[-1])
    for k, v in avg.items():
        if not v.is_floating_point():
            assert torch.equal(v, snaps[-1][k]), k  # num_batches_tracked: the live model's


@pytest.mark.parametrize("math", ["f32", "bf16io"])
@pytest.mark.parametrize("arch", list(ARCHS))
def test_validate_under_applied_equals_a_model_loaded_with_the_average(arch, math):
    model, ema, opt, snaps = trained(arch, 2, math=math)
    loader = batches(arch, 2, seed0=300)
    crit = nn.CrossEntropyLoss()
    live = validate(model, loader, crit, DEV, progress=False)  # records the eval plan on the live weights first
    with ema.applied():
        got = validate(model, loader, crit, DEV, progress=False)
    want = validate(fresh_with(arch, ema.averaged_state_dict(), math), loader, crit, DEV, progress=False)
    print(f"{arch} {math}: loss live {live['loss']!r}, averaged {got['loss']!r} / {want['loss']!r}")
    assert got["loss"] == want["loss"] and torch.equal(got["confusion"], want["confusion"])
    assert got["loss"] != live["loss"]  # the averaged model is another model
    same_state(snapshot(model), snaps[-1])  # and the live one is back, bit for bit
    again = validate(model, loader, crit, DEV, progress=False)
    assert again["loss"] == live["loss"] and torch.equal(again["confusion"], live["confusion"])
    assert model.training


@pytest.mark.parametrize("arch", list(ARCHS))
def test_predictor_refresh_under_applied(arch):
    model, ema, opt, snaps = trained(arch, 2)
    g = torch.Generator().manual_seed(8)
    frame = torch.randint(0, 256, (64, 128, 3), generator=g, dtype=torch.uint8).to(DEV)
    pred = Predictor(model, frame_hw=(64, 128), math="f16")  # folded from the live weights
    live_mask, live_logits = pred(frame).clone(), pred.logits()
    with ema.applied():
        pred.refresh()
    mask, logits = pred(frame).clone(), pred.logits()
    ref = Predictor(fresh_with(arch, ema.averaged_state_dict()), frame_hw=(64, 128), math="f16")
    want_mask, want_logits = ref(frame).clone(), ref.logits()
    assert torch.equal(mask, want_mask) and torch.equal(logits, want_logits)
    assert not torch.equal(logits, live_logits)
    same_state(snapshot(model), snaps[-1])
    pred.refresh()  # outside: the live weights again
    assert torch.equal(pred(frame), live_mask) and torch.equal(pred.logits(), live_logits)


@pytest.mark.parametrize("arch", list(ARCHS))
def test_no_trace_after_leaving_applied(arch):
    """Step, evaluate the averaged model, step -- against a twin that never swapped."""
    last = batches(arch, 1, seed0=500)
    loader = batches(arch, 1, seed0=300)
    crit = nn.CrossEntropyLoss()
    out = []
    for swapping in (True, False):
        model, ema, opt, snaps = trained(arch, 2)
        if swapping:
            with ema.applied():
                validate(model, loader, crit, DEV, progress=False)
            ema.swap()
            ema.swap()
        loss = train_one_epoch(model, last, crit, opt, DEV, progress=False, ema=ema)
        out.append((loss, snapshot(model), [e.clone() for e in ema.shadows], ema.num_updates))
    (la, sa, ea, na), (lb, sb, eb, nb) = out
    assert la == lb and na == nb == 3
    same_state(sa, sb)
    assert all(torch.equal(a, b) for a, b in zip(ea, eb))


@pytest.mark.parametrize("arch", list(ARCHS))
def test_applied_between_forward_and_backward_raises(arch):
    model, ema, opt, snaps = trained(arch, 1)
    twin, _, _, _ = trained(arch, 1)
    (x, y), = batches(arch, 1, seed0=500)
    x, y = x.to(DEV), y.to(DEV)
    shadows = [e.clone() for e in ema.shadows]
    model.zero_grad()
    twin.zero_grad()
    loss = model.forward_loss(x, y)
    after_forward = snapshot(model)  # (a train-mode forward has moved the BatchNorm statistics)
    with pytest.raises(RuntimeError):
        with ema.applied():
            pass
    with pytest.raises(RuntimeError):
        ema.swap()
    same_state(snapshot(model), after_forward)
    assert all(torch.equal(a, b) for a, b in zip(ema.shadows, shadows))
    loss.backward()  # still succeeds, on the weights its forward ran on
    ref = twin.forward_loss(x, y)
    ref.backward()
    torch.cuda.synchronize()
    assert loss.item() == ref.item()
    for (k, p), q in zip(model.named_parameters(), twin.parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    with ema.applied():  # and after the backward the exchange is allowed again
        pass
    same_state(snapshot(model), after_forward)


@pytest.mark.parametrize("arch", list(ARCHS))
def test_out_of_range_label_leaves_everything_as_it_was(arch):
    model, ema, opt, snaps = trained(arch, 1)
    shadows = [e.clone() for e in ema.shadows]
    state = [{k: v.clone() for k, v in opt.state[p].items()} for g in opt.param_groups for p in g["params"]]
    (x, y), = batches(arch, 1, seed0=500)
    bad = y.clone()
    bad[0, 0, 0] = ARCHS[arch][1]
    with pytest.raises(IndexError):
        train_one_epoch(model, [(x, bad)], nn.CrossEntropyLoss(), opt, DEV, progress=False, ema=ema)
    torch.cuda.synchronize()
    assert ema.num_updates == 1
    assert all(torch.equal(a, b) for a, b in zip(ema.shadows, shadows))
    for (k, p) in model.named_parameters():
        assert torch.equal(p, snaps[-1][k]), k
    now = [opt.state[p] for g in opt.param_groups for p in g["params"]]
    assert len(now) == len(state)
    for s0, s1 in zip(state, now):
        assert s0.keys() == s1.keys() and all(torch.equal(s0[k], s1[k]) for k in s0)
    # the next good batch is averaged in as update number 2
    train_one_epoch(model, [(x, y)], nn.CrossEntropyLoss(), opt, DEV, progress=False, ema=ema)
    torch.cuda.synchronize()
    assert ema.num_updates == 2 and any(not torch.equal(a, b) for a, b in zip(ema.shadows, shadows))


def test_frozen_backbone_shadows_stay_equal_to_their_sources():
    model = build("mnv2")
    freeze(model)
    model.train()
    ema, opt = EMA(model, decay=DECAY), optimizer(model)
    start = snapshot(model)
    for b in batches("mnv2", 2):
        train_one_epoch(model, [b], nn.CrossEntropyLoss(), opt, DEV, progress=False, ema=ema)
    sd = snapshot(model)
    frozen = [k for k in ema.names if k.startswith("backbone.")]
    assert len(frozen) > 100
    for k in frozen:
        e = ema.shadows[ema._slot[k]]
        assert torch.equal(sd[k], start[k]) and torch.equal(e, sd[k]), k
    rest = [k for k in ema.names if ema._slot[k] not in {ema._slot[f] for f in frozen}]
    assert rest and sum(int(not torch.equal(ema.shadows[ema._slot[k]], sd[k])) for k in rest) > len(rest) // 2


@pytest.fixture()
def pg():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_data_parallel_world1_follows_the_flattened_buffers(pg):
    from seg_amd.ddp import DataParallel
    batch = batches("mnv2", 1)
    crit = nn.CrossEntropyLoss()
    plain = build("mnv2")
    ema_p, opt_p = EMA(plain, decay=DECAY), optimizer(plain)
    core = build("mnv2")
    ema_w = EMA(core, decay=DECAY)  # built before the wrap: the BatchNorm statistics are rebound after it
    key = ema_w._key
    wrapped = DataParallel(core, bucket_cap_mb=1.0)
    wrapped.train()
    opt_w = optimizer(wrapped)
    train_one_epoch(plain, batch, crit, opt_p, DEV, progress=False, ema=ema_p)
    train_one_epoch(wrapped, batch, crit, opt_w, DEV, progress=False, ema=ema_w)
    torch.cuda.synchronize()
    assert ema_w._key != key  # the table was rebuilt over the flat buffer's views
    flat = wrapped._bn_flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
    stats = [i for i, (d, n) in enumerate(ema_w._where) if n in ("running_mean", "running_var")]
    assert stats and all(lo <= ema_w._key[i] < hi for i in stats)
    same_state(snapshot(plain), snapshot(wrapped))
    assert ema_p.names == ema_w.names
    for k in ema_p.names:
        assert torch.equal(ema_p.shadows[ema_p._slot[k]], ema_w.shadows[ema_w._slot[k]]), k
    live = snapshot(wrapped)
    with ema_w.applied():
        same_state(snapshot(wrapped), ema_p.averaged_state_dict())
    same_state(snapshot(wrapped), live)
