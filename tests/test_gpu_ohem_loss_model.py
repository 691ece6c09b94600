"""GPU: a seg_amd.OhemCELoss through the model -- compute_loss / validate / train_one_epoch take the fused path for
it (the seg_ohem_* kernels: the hard pixels are selected on the device, no full-resolution logits), and that path
agrees with the same engine's logits path (criterion(model(x), t): full-resolution logits, OhemCELoss's torch forward),
with which it shares every kernel below the low-resolution logit gradient.  The shape and the tolerances of
tests/test_gpu_seg_loss_model.py.

An untrained model gets every pixel wrong, so thresh = 0.7 alone would keep them all.  Each comparison therefore takes
its cut from the reference: from the logits path's per-pixel losses (in fp64, on the CPU) it picks, in the middle third
of the ranks, the floor k whose k-th largest loss has the widest clearance to its neighbours (top-k mode, under a tau
above every loss) and the tau in the widest gap between neighbours (threshold mode), and asserts that the clearance
exceeds 1e-4 -- rounding cannot move a pixel across the cut.

Measured on an MI355X.  The loss agrees to 3e-7 relative in all eight cases, and the selection (#valid, #kept) is the
reference's.  The gradient checks are tests/test_gpu_seg_loss_model.py's three, unchanged:
  * the head's weight / bias gradients within 1e-4: f32 1.0e-7 at most; mnv2-bf16io 1.2e-6 / 7.7e-7 (top-k cut) and
    6.4e-6 / 6.4e-6 (threshold cut).  The bf16io gradient twin writes the full-resolution gradient in fp32 for this:
    as bf16 rows (what the other families store; the plain-CE pair is at 2.6e-4 / 1.7e-4 on this model) it was at
    1.9e-4 / 1.2e-4;
  * every parameter within twice the plain-CE pair's worst, and the parameters with a gradient to speak of within
    twice the plain pair's worst over them: mnv2-f32 1.75e-4 and 1.36e-4 against 2 x 1.73e-4, unet-f32 1.49e-6 and
    1.25e-6 against 2 x 8.71e-7, unet-bf16io both paths bit for bit.
With K fixed the criterion is nn.CrossEntropyLoss(weight) on the labels with every pixel outside K ignored; the test
prints that pair's spread (the seg_cew_* kernels against the logits path) beside OHEM's.  In f32 the two fused sides
are bitwise equal (tests/test_gpu_ohem_loss.py asserts it on the kernels).
"""
import math
import os
import socket

import pytest
import torch
from torch import nn

from seg_amd import Adam, MobileNetV2UNet, OhemCELoss, UNet, engine, train_one_epoch, validate
from seg_amd.detinit import deterministic_init, synthetic_batch
from seg_amd.losses import ohem_loss_terms
from seg_amd.train import compute_loss, fused_loss_options

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 10
GAP = 1e-4


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def make(kind="mnv2", seed=1, train=False, conv_math="f32"):
    net = MobileNetV2UNet(C) if kind == "mnv2" else UNet(C, 8)
    m = deterministic_init(net, seed=seed, random_running_stats=True).to(DEV)
    engine.set_conv_math(m, conv_math)
    return m.train() if train else m.eval()


def class_w(seed=5):
    return torch.rand(C, generator=torch.Generator().manual_seed(seed)) * 3 + 0.05


def batch(n=2, seed=7):
    x, y = synthetic_batch(n, 64, 64, C, seed=seed)
    y[0, :3] = -100
    return x.to(DEV), y.to(DEV)


def grads_of(model, loss_fn):
    model.zero_grad(set_to_none=True)
    loss = loss_fn()
    loss.backward()
    return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def cuts(model, x, t):
    """{mode: (thresh, k)} with the clearance asserted, from the logits path's losses (module docstring)."""
    with torch.no_grad():
        z = model(x).double().cpu()
    l = nn.functional.cross_entropy(z, t.cpu(), reduction="none")[t.cpu() != -100].sort(descending=True).values
    n = l.numel()
    a, b = n // 3, 2 * n // 3
    gaps = l[:-1] - l[1:]                                     # gaps[i]: between ranks i and i + 1 (0-based)
    clear = torch.minimum(gaps[a - 1:b - 1], gaps[a:b])       # of rank i in [a, b): to both neighbours
    i = a + int(clear.argmax())
    j = a + int(gaps[a:b].argmax())
    tau = float(l[j] + l[j + 1]) / 2
    assert float(clear.max()) > GAP and float(gaps[j]) / 2 > GAP, (float(clear.max()), float(gaps[j]))
    assert float(l[0]) < 30.0
    return {"topk": (math.exp(-40.0), i + 1), "threshold": (math.exp(-tau), max(j // 4, 1))}


@pytest.mark.parametrize("conv_math", ["f32", "bf16io"])
@pytest.mark.parametrize("kind", ["mnv2", "unet"])
def test_loss_and_gradients_fused_against_logits_path(kind, conv_math, record):
    # train(): the engine has no backward through eval-mode BatchNorm; the forward is the same launches in both paths
    model = make(kind, train=True, conv_math=conv_math)
    x, t = batch()
    last = [m for m in model.modules() if isinstance(m, nn.Conv2d)][-1]
    names = {id(p): k for k, p in model.named_parameters()}
    plain = nn.CrossEntropyLoss()
    _, gf = grads_of(model, lambda: compute_loss(model, plain, x, t))
    _, gl = grads_of(model, lambda: plain(model(x), t))
    assert gf.keys() == gl.keys() and len(gf) > (100 if kind == "mnv2" else 30)
    # the plain criterion's fused-vs-logits spread per parameter is the yardstick, as in
    # tests/test_gpu_seg_loss_model.py
    plain_rel = {k: rel(gf[k], gl[k]) for k in gf}
    worst = max(plain_rel.values())
    nv = int((t != -100).sum())
    print(f"{kind} {conv_math} plain CE: worst {worst:.3e}, head {plain_rel[names[id(last.weight)]]:.3e} "
          f"{plain_rel[names[id(last.bias)]]:.3e}")
    missed = []
    for mode, (thresh, k) in cuts(model, x, t).items():
        crit = OhemCELoss(thresh, k, weight=class_w()).to(DEV)
        lf, wf = grads_of(model, lambda: compute_loss(model, crit, x, t))
        stats = model.__dict__["_segamd_last_stats"].clone()
        ll, wl = grads_of(model, lambda: crit(model(x), t))
        kept = int(stats[4].item())
        assert stats[3].item() == nv and (kept == k if mode == "topk" else k <= kept < nv), (mode, stats, k)
        assert abs(lf.item() - ll.item()) <= 1e-5 * abs(ll.item()), (mode, lf.item(), ll.item())
        w_rel = {p: rel(wf[p], wl[p]) for p in wf}
        hw, hb = w_rel[names[id(last.weight)]], w_rel[names[id(last.bias)]]
        top = max(float(g.norm()) for g in wl.values())
        real = [p for p in wl if float(wl[p].norm()) > 1e-6 * top and float(gl[p].norm()) > 1e-6 * top]
        worst_real, w_worst_real = max(plain_rel[p] for p in real), max(w_rel[p] for p in real)
        record(kind=kind, math=conv_math, mode=mode, thresh=thresh, k=k, kept=kept, loss_fused=lf.item(),
               loss_logits=ll.item(), plain_worst=worst, ohem_worst=max(w_rel.values()), head_weight=hw, head_bias=hb,
               plain_worst_nonzero=worst_real, ohem_worst_nonzero=w_worst_real, nonzero_params=len(real))
        print(f"{kind} {conv_math} {mode}: k {k} kept {kept} of {nv}, loss {lf.item():.6f} / {ll.item():.6f}, plain "
              f"worst {worst:.3e}, OHEM worst {max(w_rel.values()):.3e}, head {hw:.3e} {hb:.3e}, non-zero gradients "
              f"({len(real)}): plain worst {worst_real:.3e}, OHEM worst {w_worst_real:.3e}")
        # for the record, not asserted: with K fixed the criterion IS nn.CrossEntropyLoss(weight) on the labels with
        # every pixel outside K ignored -- the spread of that pair (the seg_cew_* kernels against the logits path)
        with torch.no_grad():
            kept_mask = ohem_loss_terms(model(x), t, thresh, k, crit.weight)[1]
        tk = torch.where(kept_mask, t, torch.full_like(t, -100))
        cew = nn.CrossEntropyLoss(weight=crit.weight)
        _, mf = grads_of(model, lambda: compute_loss(model, cew, x, tk))
        _, ml = grads_of(model, lambda: cew(model(x), tk))
        m_rel = {p: rel(mf[p], ml[p]) for p in mf}
        print(f"{kind} {conv_math} {mode}: weighted CE on the labels masked to K, fused against logits: worst "
              f"{max(m_rel.values()):.3e}, non-zero gradients worst {max(m_rel[p] for p in real):.3e}, head "
              f"{m_rel[names[id(last.weight)]]:.3e} {m_rel[names[id(last.bias)]]:.3e}; OHEM against it, fused: "
              f"{max(rel(wf[p], mf[p]) for p in real):.3e}")
        if not (hw < 1e-4 and hb < 1e-4):
            missed.append((mode, "head", hw, hb))
        missed += [(mode, p, v, worst) for p, v in w_rel.items() if not v <= 2 * worst]
        assert len(real) > (100 if kind == "mnv2" else 30)
        if not w_worst_real <= 2 * worst_real:
            missed.append((mode, "non-zero gradients", w_worst_real, worst_real))
    assert not missed, missed


def test_no_full_resolution_logits_and_the_workspace():
    """With its plan recorded, a fused OHEM step allocates at least one set of full-resolution logits less than the
    same step on the logits path; the plan's loss workspace is 4 B per pixel plus the select's few KB."""
    x, t = batch()
    crit = OhemCELoss(0.7, 1 / 16).to(DEV)
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
    plan = next(p for p in tm.__dict__["_segamd_plans"].values() if p.mode == "loss")
    pixels = t.numel()
    tau, work = plan.run.ohem
    assert tau == -math.log(0.7) and work.numel() * 4 <= 4 * pixels + 64 * 1024


def test_three_steps_with_different_targets_each_give_their_own_loss():
    """The tape replays the launch sequence on one workspace, which every call clears: other labels, other value."""
    model = make()
    x, _ = batch()
    ts = [batch(seed=s)[1] for s in (7, 8, 9)]
    crit = OhemCELoss(math.exp(-40.0), 0.4, weight=class_w()).to(DEV)  # top-k mode: the refine passes run
    got, ref = [], []
    with torch.no_grad():
        for t in ts + ts[:1]:
            got.append(compute_loss(model, crit, x, t).item())
            st = model.__dict__["_segamd_last_stats"]
            assert st[4].item() >= int(0.4 * t.numel()) and st[5].item() < 40.0
        for t in ts:
            ref.append(crit(model(x), t).item())
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-5 * abs(r), (got, ref)
    assert len({round(r, 6) for r in ref}) == 3 and got[3] == got[0]
    assert len([k for k, p in model.__dict__["_segamd_plans"].items() if p.mode == "loss"]) == 1


def test_validate_with_an_ohem_loss():
    model = make()
    crit = OhemCELoss(math.exp(-40.0), 0.25, weight=class_w()).to(DEV)
    loader = [batch(seed=7), batch(seed=8)]
    r = validate(model, loader, crit, DEV, progress=False)
    assert engine.bad_label_count(model) is not None
    with torch.no_grad():
        ref = sum(crit(model(x), t).item() for x, t in loader) / len(loader)
    assert abs(r["loss"] - ref) <= 1e-5 * abs(ref)
    r0 = validate(model, loader, nn.CrossEntropyLoss(), DEV, progress=False)
    assert torch.equal(r["confusion"], r0["confusion"]) and r["miou"] == r0["miou"]
    assert r["loss"] > r0["loss"]  # the mean over the hardest quarter
    assert int(r["confusion"].sum()) == sum(int((t != -100).sum()) for _, t in loader)


def test_train_one_epoch_skips_the_step_on_an_out_of_range_label():
    model = make(train=True)
    crit = OhemCELoss(0.7, 1 / 16).to(DEV)
    x, t = batch()
    t[1, 5, 5] = C
    opt = Adam(model.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    with pytest.raises(IndexError, match="Target out of bounds"):
        train_one_epoch(model, [(x, t)], crit, opt, DEV, progress=False)
    for k, v in model.named_parameters():
        assert torch.equal(v, before[k]), k
    for st in opt.state.values():
        assert st["step"].item() == 0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    t[1, 5, 5] = 3
    assert train_one_epoch(model, [(x, t)], crit, opt, DEV, progress=False) > 0
    assert all(st["step"].item() == 1 for st in opt.state.values())
    assert any(not torch.equal(v, before[k]) for k, v in model.named_parameters())


@pytest.mark.parametrize("conv_math", ["f32", "bf16io"])
def test_train_one_epoch_lowers_the_loss_of_a_repeated_batch(conv_math):
    model = make(train=True, conv_math=conv_math)
    crit = OhemCELoss(0.7, 1 / 16, weight=class_w()).to(DEV)
    opt = Adam(model.parameters(), lr=1e-3)
    data = [batch(seed=7), batch(seed=7)]
    first = train_one_epoch(model, data[:1], crit, opt, DEV, progress=False)
    for _ in range(3):
        last = train_one_epoch(model, data, crit, opt, DEV, progress=False)
    assert math.isfinite(first) and last < first, (first, last)
    assert fused_loss_options(crit)["ohem_min_kept"] == 1 / 16


def test_option_validation():
    model = make()
    x, t = batch(1)
    for kw in (dict(ohem_thresh=0.7), dict(ohem_min_kept=10), dict(ohem_thresh=1.0, ohem_min_kept=10),
               dict(ohem_thresh=0.7, ohem_min_kept=0), dict(ohem_thresh=0.7, ohem_min_kept=10, label_smoothing=0.1),
               dict(ohem_thresh=0.7, ohem_min_kept=10, reduction="sum"),
               dict(ohem_thresh=0.7, ohem_min_kept=10, dice=1.0)):
        with pytest.raises(ValueError):
            model.forward_loss(x, t, **kw)
        with pytest.raises(ValueError):
            model.forward_metrics(x, t, torch.zeros(C, C, dtype=torch.int64, device=DEV), **kw)
    assert torch.isfinite(model.forward_loss(x, t, ohem_thresh=0.7, ohem_min_kept=0.5, weight=class_w().to(DEV)))


@pytest.fixture
def pg():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_data_parallel_world1_is_bitwise_the_plain_model(pg):
    from seg_amd.ddp import DataParallel
    x, t = batch()
    crit = OhemCELoss(math.exp(-40.0), 0.3, weight=class_w()).to(DEV)
    res = []
    for wrap in (False, True):
        m = make(seed=9, train=True)
        model = DataParallel(m, bucket_cap_mb=1.0) if wrap else m
        out = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            loss = compute_loss(model, crit, x, t)
            loss.backward()
            if wrap:
                model.finish_gradient_sync()
            out.append((loss.detach().clone(),
                        {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
        res.append(out)
    for (lp, gp), (lw, gw) in zip(*res):
        assert torch.equal(lp.view(torch.int32), lw.view(torch.int32))
        assert gp.keys() == gw.keys() and len(gp) > 100
        for k in gp:
            assert torch.equal(gp[k], gw[k]), k
