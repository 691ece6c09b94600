"""GPU: a seg_amd.SegLoss (focal exponent, soft Dice term) through the model -- compute_loss / validate /
train_one_epoch take the fused path for it, and that path agrees with the same engine's logits path
(criterion(model(x), t): full-resolution logits, SegLoss's torch forward), with which it shares every kernel below
the low-resolution logit gradient.  The shape of tests/test_gpu_loss_options_model.py.
"""
import pytest
import torch
from torch import nn

from seg_amd import AdamW, MobileNetV2UNet, SegLoss, engine, train_one_epoch, validate
from seg_amd.detinit import deterministic_init, synthetic_batch
from seg_amd.train import compute_loss, fused_loss_options

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 10


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def make(seed=1, train=False):
    m = deterministic_init(MobileNetV2UNet(C), seed=seed, random_running_stats=True).to(DEV)
    return m.train() if train else m.eval()


def class_w(seed=5):
    return torch.rand(C, generator=torch.Generator().manual_seed(seed)) * 3 + 0.05


def criterion(w=None, **kw):
    kw = {"ce": 1.0, "dice": 1.0, "focal_gamma": 2.0, **kw}
    return SegLoss(weight=class_w() if w is None else w, **kw).to(DEV)


def batch(n=2, seed=7):
    x, y = synthetic_batch(n, 64, 64, C, seed=seed)
    y[0, :3] = -100
    return x.to(DEV), y.to(DEV)


def grads_of(model, loss_fn):
    model.zero_grad(set_to_none=True)
    loss = loss_fn()
    loss.backward()
    return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_compute_loss_takes_the_fused_path():
    model, crit = make(), criterion()
    x, t = batch()
    assert engine.bad_label_count(model) is None
    with torch.no_grad():
        loss = compute_loss(model, crit, x, t)
        assert engine.bad_label_count(model) is not None  # the logits path clears it
        assert engine.bad_label_count(model).item() == 0
        ref = crit(model(x), t)
        assert engine.bad_label_count(model) is None
        assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    # no full-resolution logits: with its plan recorded, a fused training step (forward + backward) allocates at
    # least one set of them less than the same step on the logits path
    full = x.shape[0] * C * x.shape[2] * x.shape[3] * 4
    tm = make(train=True)
    grown = {}
    for name, fn in (("fused", lambda: compute_loss(tm, crit, x, t)), ("logits", lambda: crit(tm(x), t))):
        for k in range(2):  # record, then measure a replay
            tm.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn().backward()
            torch.cuda.synchronize()
            grown[name] = torch.cuda.max_memory_allocated() - base
    print("a step allocates", grown, "bytes; full-resolution logits", full)
    assert grown["fused"] + full <= grown["logits"], (grown, full)
    # each term on its own, label smoothing beside the Dice term, another ignore_index (for which -100 would be an
    # out-of-range label: those pixels become class 2, the ignored one)
    t2 = torch.where(t == -100, torch.full_like(t, 2), t)
    for c, tc in ((SegLoss(focal_gamma=0.5), t), (SegLoss(ce=0.0, dice=1.0), t), (SegLoss(ce=0.5), t),
                  (SegLoss(dice=0.5, label_smoothing=0.1, weight=class_w()), t),
                  (SegLoss(ce=0.3, dice=2.0, focal_gamma=1.0, weight=class_w(), ignore_index=2, dice_smooth=0.1), t2)):
        c = c.to(DEV)
        with torch.no_grad():
            loss, ref = compute_loss(model, c, x, tc), c(model(x), tc)
        assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), c


def test_gradients_fused_against_logits_path(record):
    # train(): the engine has no backward through eval-mode BatchNorm; the forward is the same launches in both paths
    model = make(train=True)
    x, t = batch()
    last = [m for m in model.modules() if isinstance(m, nn.Conv2d)][-1]
    names = {id(p): k for k, p in model.named_parameters()}
    plain = nn.CrossEntropyLoss()
    _, gf = grads_of(model, lambda: compute_loss(model, plain, x, t))
    _, gl = grads_of(model, lambda: plain(model(x), t))
    assert gf.keys() == gl.keys() and len(gf) > 100
    # the plain criterion's fused-vs-logits spread per parameter is the yardstick, as in
    # tests/test_gpu_loss_options_model.py (its comment says which parameters hold rounding noise only)
    plain_rel = {k: rel(gf[k], gl[k]) for k in gf}
    worst = max(plain_rel.values())
    crit = criterion()
    lf, wf = grads_of(model, lambda: compute_loss(model, crit, x, t))
    ll, wl = grads_of(model, lambda: crit(model(x), t))
    assert abs(lf.item() - ll.item()) <= 1e-5 * abs(ll.item())
    w_rel = {k: rel(wf[k], wl[k]) for k in wf}
    record(plain_worst=worst, plain_worst_param=max(plain_rel, key=plain_rel.get),
           segloss_worst=max(w_rel.values()), segloss_worst_param=max(w_rel, key=w_rel.get),
           head_weight=w_rel[names[id(last.weight)]], head_bias=w_rel[names[id(last.bias)]])
    print(f"plain worst {worst:.3e}, SegLoss worst {max(w_rel.values()):.3e}, "
          f"head {w_rel[names[id(last.weight)]]:.3e} {w_rel[names[id(last.bias)]]:.3e}")
    assert w_rel[names[id(last.weight)]] < 1e-4 and w_rel[names[id(last.bias)]] < 1e-4
    for k, v in w_rel.items():
        assert v <= 2 * worst, (k, v, worst)
    top = max(float(g.norm()) for g in wl.values())
    real = [k for k in wl if float(wl[k].norm()) > 1e-6 * top and float(gl[k].norm()) > 1e-6 * top]
    assert len(real) > 100
    worst_real, w_worst_real = max(plain_rel[k] for k in real), max(w_rel[k] for k in real)
    record(plain_worst_nonzero=worst_real, segloss_worst_nonzero=w_worst_real, nonzero_params=len(real))
    print(f"non-zero gradients ({len(real)}): plain worst {worst_real:.3e}, SegLoss worst {w_worst_real:.3e}")
    assert w_worst_real <= 2 * worst_real


def test_two_steps_with_different_scalars_each_give_their_own_loss():
    model = make()
    x, t = batch()
    crits = [criterion(focal_gamma=2.0, dice=1.0), criterion(focal_gamma=0.5, dice=0.25),
             criterion(focal_gamma=2.0, dice=1.0)]
    got, ref = [], []
    with torch.no_grad():
        for c in crits:
            got.append(compute_loss(model, c, x, t).item())
        for c in crits:
            ref.append(c(model(x), t).item())
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-5 * abs(r), (got, ref)
    assert abs(ref[0] - ref[1]) > 1e-3 * abs(ref[0]) and got[0] == got[2]
    keys = [k for k, p in model.__dict__["_segamd_plans"].items() if p.mode == "loss"]
    assert len(keys) == 2  # one plan per (gamma, dice), the third step reused the first


def test_weight_values_and_weight_tensor_may_change_without_a_new_plan():
    model, crit = make(), criterion()
    x, t = batch()

    def both():
        with torch.no_grad():
            return compute_loss(model, crit, x, t).item(), crit(model(x), t).item()

    l0, r0 = both()
    assert abs(l0 - r0) <= 1e-5 * abs(r0)
    fwd = {k: p.fwd for k, p in model.__dict__["_segamd_plans"].items()}
    assert len(fwd) == 2  # the fused-loss plan and the logits plan
    with torch.no_grad():
        crit.weight.mul_(0.25)
        crit.weight[3] = 4.0
    l1, r1 = both()
    assert abs(l1 - r1) <= 1e-5 * abs(r1) and abs(r1 - r0) > 1e-3 * abs(r0)
    crit.weight = class_w(seed=9).to(DEV)  # another tensor
    l2, r2 = both()
    assert abs(l2 - r2) <= 1e-5 * abs(r2) and abs(r2 - r1) > 1e-3 * abs(r1)
    assert {k: p.fwd for k, p in model.__dict__["_segamd_plans"].items()} == fwd


def test_validate_with_a_seg_loss():
    model, crit = make(), criterion()
    loader = [batch(seed=7), batch(seed=8)]
    r = validate(model, loader, crit, DEV, progress=False)
    assert engine.bad_label_count(model) is not None
    with torch.no_grad():
        ref = sum(crit(model(x), t).item() for x, t in loader) / len(loader)
    assert abs(r["loss"] - ref) <= 1e-5 * abs(ref)
    r0 = validate(model, loader, nn.CrossEntropyLoss(), DEV, progress=False)
    assert torch.equal(r["confusion"], r0["confusion"]) and r["miou"] == r0["miou"]
    assert r["loss"] != r0["loss"]
    # the validation forward replays its recorded plan: it allocates less than one set of full-resolution logits
    x, t = loader[0]
    cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    opts = fused_loss_options(crit)
    model.forward_metrics(x, t, cm, **opts)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    model.forward_metrics(x, t, cm, **opts)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < x.shape[0] * C * x.shape[2] * x.shape[3] * 4, grown
    assert int(r["confusion"].sum()) == sum(int((t != -100).sum()) for _, t in loader)


def test_train_one_epoch_skips_the_step_on_an_out_of_range_label():
    model, crit = make(train=True), criterion()
    x, t = batch()
    t[1, 5, 5] = C
    opt = AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    with pytest.raises(IndexError, match="Target out of bounds"):
        train_one_epoch(model, [(x, t)], crit, opt, DEV, progress=False, max_grad_norm=1.0)
    for k, v in model.named_parameters():
        assert torch.equal(v, before[k]), k
    for st in opt.state.values():
        assert st["step"].item() == 0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    t[1, 5, 5] = 3
    assert train_one_epoch(model, [(x, t)], crit, opt, DEV, progress=False, max_grad_norm=1.0) > 0
    assert all(st["step"].item() == 1 for st in opt.state.values())
    assert any(not torch.equal(v, before[k]) for k, v in model.named_parameters())


def test_option_validation():
    model = make()
    x, t = batch(1)
    for kw in (dict(ce=-1.0), dict(dice=-1.0), dict(focal_gamma=-0.5), dict(ce=0.0), dict(dice=1.0, dice_smooth=0.0),
               dict(focal_gamma=2.0, label_smoothing=0.1), dict(dice=1.0, reduction="sum")):
        with pytest.raises(ValueError):
            model.forward_loss(x, t, **kw)
        with pytest.raises(ValueError):
            model.forward_metrics(x, t, torch.zeros(C, C, dtype=torch.int64, device=DEV), **kw)
    assert torch.isfinite(model.forward_loss(x, t, dice=1.0, focal_gamma=2.0, weight=class_w().to(DEV)))


@pytest.mark.parametrize("math", ["f32", "bf16io"])
def test_tape_replay_equals_immediate_walk(math):
    """tests/test_gpu_tape.py's comparison with a SegLoss's options on: a Run without a recorder issues every launch
    on the spot, the model's forward_loss replays the recorded tapes."""
    model = make(seed=2, train=True)
    engine.set_conv_math(model, math)
    w = class_w().to(DEV)
    sl = dict(ce=0.7, dice=1.3, focal_gamma=1.5, dice_smooth=0.5)
    for step in range(3):  # record, then two replays with new input tensors
        x, y = synthetic_batch(2, 64, 64, C, seed=50 + step)
        x, y = x.to(DEV), y.to(DEV)
        bufs = {k: b.clone() for k, b in model.named_buffers()}
        prog = engine.get_program(model, *x.shape[:1], *x.shape[2:])
        run = engine.Run(prog, x.contiguous(), True)
        run.forward()
        stats = engine._loss_forward(run, y, -100, weight=w, sl=tuple(sl.values()))
        engine._loss_backward(run, torch.ones(1, device=DEV), -100)
        le = stats[0].clone()
        ge = {k: run.grads[id(p)].clone() for k, p in model.named_parameters() if id(p) in run.grads}
        for k, b in model.named_buffers():
            b.copy_(bufs[k])
        lt, gt = grads_of(model, lambda: model.forward_loss(x, y, weight=w, **sl))
        torch.cuda.synchronize()
        assert torch.equal(le.view(torch.int32), lt.view(torch.int32)), (step, le.item(), lt.item())
        assert ge.keys() == gt.keys()
        for k in ge:
            assert torch.equal(ge[k], gt[k]), (step, k)
