"""GPU: fine-tuning on the HIP engine -- frozen BatchNorm statistics, frozen parameters, the truncated backward.

Gradient checks are the three-part check of oracle/budget.py, restated here for a forward composed from the oracle's
own blocks with a training flag per block (segref.mobilenet_features(p, x, False), segref.up(..., True), ...):
  1. every activation layer's pre-activation z of the HIP forward within budget.Z_FACTOR x the oracle's own fp32
     error of that layer;
  2. the fp64 oracle re-run with the HIP path's own ReLU / ReLU6 masks (and max-pool choices): g64m;
  3. per tensor ||g_hip - g64m|| <= max(1e-3 ||g64m||, 4 eps_ref, 1e-4 ||G64||), eps_ref = the oracle's fp32 error
     with the fp64 masks forced.
Nothing is sized from the HIP result.  Shapes: MobileNetV2UNet(10) at 2x3x64x64, UNet(4) at 2x3x32x64, running
statistics randomised (mean +-0.2, variance 0.5..1.5) so that frozen and batch statistics differ.
"""
import os
import socket

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import budget, segref
from seg_amd import MobileNetV2UNet, UNet, engine, freeze, unfreeze
from seg_amd.detinit import deterministic_init, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def build(ctor=lambda: MobileNetV2UNet(10), seed=11):
    """A CPU model with deterministic weights and randomised running statistics."""
    m = deterministic_init(ctor(), seed=seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.rand(mod.num_features, generator=g) * 0.4 - 0.2)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return m


def named_grads(model):
    out, seen = {}, set()
    for k, p in model.named_parameters():
        if id(p) not in seen and p.grad is not None:
            out[k] = p.grad.detach().clone()
        seen.add(id(p))
    return out


def buffers(model):
    return {k: b.detach().clone() for k, b in model.named_buffers()}


def step(model, x, y, **opts):
    model.zero_grad(set_to_none=True)
    loss = model.forward_loss(x, y, **opts)
    loss.backward()
    sync = getattr(model, "finish_gradient_sync", None)
    if sync is not None:
        sync()
    torch.cuda.synchronize()
    return loss.detach().clone(), named_grads(getattr(model, "module", model))


def hip_step(model, x, y):
    """One fused-loss step keeping the run: (loss, gradients, pre-activations, max-pool choices)."""
    engine.DEBUG_KEEP_RUN = True
    try:
        loss, g = step(model, x, y)
        z, pools = engine.debug_preactivations(model), engine.debug_pool_positions(model)
    finally:
        engine.DEBUG_KEEP_RUN, engine.LAST_RUN = False, None
    return loss, g, z, pools


def mnv2_forward(backbone_training, decoder_training=True):
    def fwd(p, x):
        f = segref.mobilenet_features(p, x, backbone_training)
        t = decoder_training
        y = segref.up(p, "up1.", f[18], f[10], t)
        y = segref.up(p, "up2.", y, f[6], t)
        y = segref.up(p, "up3.", y, f[3], t)
        y = segref.up(p, "up4.", y, f[1], t)
        y = segref.outconv(p, "outc.", y, t)
        return F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=True)
    return fwd


def unet_forward_inc_down1_frozen(p, x):
    x1 = segref.double_conv(p, "inc.conv.", x, False)
    x2 = segref.double_conv(p, "down1.mpconv.1.", segref._pool("down1.", x1), False)
    x3 = segref.double_conv(p, "down2.mpconv.1.", segref._pool("down2.", x2), True)
    x4 = segref.double_conv(p, "down3.mpconv.1.", segref._pool("down3.", x3), True)
    y = segref.up(p, "up1.", x4, x3, True)
    y = segref.up(p, "up2.", y, x2, True)
    y = segref.up(p, "up3.", y, x1, True)
    return segref.outconv(p, "sem_out.", y, True)


def _oracle(fwd, names, state, x, y, dtype, masks=None, pools=None):
    p = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in state.items()}
    for k in names:
        p[k].requires_grad_(True)
    segref.MASK_OVERRIDE, segref.POOL_OVERRIDE, saved = masks, pools, segref.RECORD
    segref.RECORD = {}
    try:
        loss = F.cross_entropy(fwd(p, x.to(dtype)), y)
        z = {k[:-1]: v.detach() for k, v in segref.RECORD.items() if k.endswith(".z")}
        loss.backward()
    finally:
        segref.MASK_OVERRIDE = segref.POOL_OVERRIDE = None
        segref.RECORD = saved
    return loss.detach(), z, {k: p[k].grad.detach().clone() for k in names}


def three_part_check(fwd, names, model_cpu, x, y, hip_grads, hip_z, hip_pools=None):
    """oracle/budget.py's check for the composition `fwd` and the parameters `names`; returns (loss64, g64)."""
    state = segref.canonical_state(model_cpu.state_dict())
    _, z32, _ = _oracle(fwd, names, state, x, y, torch.float32)
    loss64, z64, g64 = _oracle(fwd, names, state, x, y, torch.float64)
    hi = dict(segref.ACT_HI)
    m64 = {k: segref.act_mask(z, hi[k]) for k, z in z64.items()}
    _, _, g32m = _oracle(fwd, names, state, x, y, torch.float32, m64)
    assert set(z64) <= set(hip_z), sorted(set(z64) - set(hip_z))[:5]
    masks, zworst = {}, 0.0
    for k, z in z64.items():
        zh = hip_z[k].double().cpu()
        err, lim = float((zh - z).abs().max()), budget.Z_FACTOR * float((z32[k].double() - z).abs().max()) + 1e-30
        zworst = max(zworst, err / lim)
        assert err <= lim, (k, err, lim)
        masks[k] = segref.act_mask(zh, hi[k])
    _, _, g64m = _oracle(fwd, names, state, x, y, torch.float64, masks, hip_pools)
    gnorm = float(torch.sqrt(sum((g ** 2).sum() for g in g64.values())))
    worst, bad = (0.0, None), []
    for k in names:
        assert k in hip_grads, f"missing gradient {k}"
        d = float((hip_grads[k].double().cpu() - g64m[k]).norm())
        tol = max(1e-3 * float(g64m[k].norm()), 4 * float((g32m[k].double() - g64[k]).norm()), 1e-4 * gnorm)
        worst = max(worst, (d / tol, k))
        if d > tol:
            bad.append((k, d, tol))
    print(f"worst gradient {worst[0]:.3f} of its bound ({worst[1]}), z within {zworst:.3f} of its bound, "
          f"{sum(int((masks[k] != m64[k]).sum()) for k in m64)} mask flips")
    assert not bad, bad[:8]
    return float(loss64), g64


@pytest.fixture(scope="module")
def data():
    x, y = synthetic_batch(2, 64, 64, 10, seed=111)
    return x, y, x.to(DEV), y.to(DEV)


def decoder_names(state):
    return [k for k in segref.trainable_names(state) if not k.startswith("backbone.")]


def test_all_batchnorm_frozen_all_parameters_trainable(data):
    x, y, xg, yg = data
    cpu = build()
    model = build().to(DEV).train()
    freeze(model, [n for n, _ in model.named_children()], params=False)
    assert model.training and not any(m.training for m in model.modules() if isinstance(m, nn.BatchNorm2d))
    before = buffers(model)
    loss, g, z, _ = hip_step(model, xg, yg)
    state = segref.canonical_state(cpu.state_dict())
    names = segref.trainable_names(state)
    # = segref.preactivations(..., training=False) / segref.forward_backward(..., False)
    loss64, g64 = three_part_check(mnv2_forward(False, False), names, cpu, x, y, g, z)
    assert abs(loss.item() - loss64) <= 1e-3 * abs(loss64)
    # a conv bias in front of a frozen BatchNorm has a real gradient, sum(dY)
    for k in ("up1.conv.conv.0.bias", "up4.conv.conv.3.bias", "outc.conv.0.bias"):
        assert float(g64[k].norm()) > 0 and float(g[k].norm()) > 0
    after = buffers(model)
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_backbone_frozen_recipe(data):
    x, y, xg, yg = data
    cpu = build()
    model = freeze(build().to(DEV)).train()
    before = buffers(model)
    inside = {id(b) for b in model.backbone.buffers()}
    loss, g, z, _ = hip_step(model, xg, yg)
    names = decoder_names(segref.canonical_state(cpu.state_dict()))
    assert sorted(g) == sorted(names)
    loss64, _ = three_part_check(mnv2_forward(False), names, cpu, x, y, g, z)
    assert abs(loss.item() - loss64) <= 1e-3 * abs(loss64)
    assert all(p.grad is None for p in model.backbone.parameters())
    changed = 0
    for k, b in model.named_buffers():
        if id(b) in inside:
            assert torch.equal(b, before[k]), k          # bitwise, num_batches_tracked included
        elif k.endswith("num_batches_tracked"):
            assert int(b) == int(before[k]) + 1, k
        else:
            assert not torch.equal(b, before[k]), k
            changed += 1
    assert changed == 2 * 9  # the decoder's nine BatchNorm layers


def grad_plan(model):
    plans = [p for p in model.__dict__["_segamd_plans"].values() if p.needs_grad and p.bwd is not None]
    assert len(plans) == 1
    return plans[0]


def test_truncation_is_exact_and_records_fewer_launches(data):
    _, _, xg, yg = data
    cut = freeze(build().to(DEV)).train()                              # no gradients for the backbone
    full = freeze(build().to(DEV), "backbone", params=False).train()   # the same forward, the whole backward
    _, gc = step(cut, xg, yg)
    _, gf = step(full, xg, yg)
    assert set(gc) < set(gf) and len(gf) == 194 and not any(k.startswith("backbone.") for k in gc)
    for k in gc:
        assert torch.equal(gc[k], gf[k]), k
    launches = lambda m: len(grad_plan(m).bwd.timers)  # noqa: E731 -- one per recorded kernel launch
    print(f"backward launches: frozen backbone {launches(cut)}, full {launches(full)}")
    assert launches(cut) < launches(full) // 2
    labels = {t[3] for t in grad_plan(cut).bwd.timers}
    assert not any(l.endswith(":bwd") and int(l.split(":")[0]) < 53 for l in labels)  # nothing below up1's conv


@pytest.mark.parametrize("bn_frozen", [False, True])
def test_frozen_convs_under_trainable_batchnorm_affine(data, bn_frozen):
    """Only the backbone's conv weights frozen: every other gradient is bitwise the full backward's.  The stem has
    nothing trainable upstream, so its BatchNorm backward writes no dY (the reduction alone: seg_bn_bwd_coef in
    train mode, seg_bn_frozen_backward without dy on frozen statistics); the other convs skip their weight
    gradients and keep their data gradients."""
    _, _, xg, yg = data
    ref, cut = build().to(DEV).train(), build().to(DEV).train()
    if bn_frozen:
        freeze(ref, "backbone", params=False)
        freeze(cut, "backbone", params=False)
    convs = [m for m in cut.backbone.features.modules() if isinstance(m, nn.Conv2d)]
    for m in convs:
        m.requires_grad_(False)
    _, gr = step(ref, xg, yg)
    _, gc = step(cut, xg, yg)
    assert len(gr) == 194 and len(gc) == 194 - len(convs) and set(gc) < set(gr)
    for k in gc:
        assert torch.equal(gc[k], gr[k]), k
    labels = [t for t in grad_plan(cut).bwd.timers if t[3] == "0:bwd"]
    assert len(labels) == 1 and labels[0][4] in ("seg_bn_bwd_coef", "seg_bn_frozen_backward")


def test_unfreeze_records_anew_and_freezing_again_reuses_the_plan(data):
    _, _, xg, yg = data
    model = freeze(build().to(DEV)).train()
    _, g1 = step(model, xg, yg)
    plans = model.__dict__["_segamd_plans"]
    first = dict(plans)
    unfreeze(model)
    stats = buffers(model)
    _, g2 = step(model, xg, yg)
    with torch.no_grad():  # the unfrozen step moved the backbone's running statistics: back in place, for step 3
        for k, b in model.named_buffers():
            b.copy_(stats[k])
    assert len(plans) == 2
    _, gfresh = step(build().to(DEV).train(), xg, yg)
    assert g2.keys() == gfresh.keys() and len(g2) == 194
    for k in g2:
        assert torch.equal(g2[k], gfresh[k]), k
    freeze(model)
    _, g3 = step(model, xg, yg)
    assert len(plans) == 2 and all(plans[k] is p and plans[k].bwd is p.bwd for k, p in first.items())
    assert g3.keys() == g1.keys()
    for k in g1:
        assert torch.equal(g1[k], g3[k]), k


def test_bf16io_backbone_frozen(data):
    """The relation tests/test_gpu_bf16.py::test_model_bf16_vs_oracle holds the train-mode bf16io model to, on the
    decoder's gradients: against the fp64 oracle, each tensor within 6x the emulated reference's own bf16 error
    (segref.bf16_convs) + 1e-3 of its norm + 1e-4 of the global norm; loss within 3x the reference's + 1e-3."""
    x, y, xg, yg = data
    cpu = build()
    state = segref.canonical_state(cpu.state_dict())
    names = decoder_names(state)
    fwd = mnv2_forward(False)
    l64, _, g64 = _oracle(fwd, names, state, x, y, torch.float64)
    with segref.bf16_convs():
        le, _, ge = _oracle(fwd, names, state, x, y, torch.float64)
    model = freeze(build().to(DEV)).train()
    engine.set_conv_math(model, "bf16io")
    before = buffers(model)
    inside = {id(b) for b in model.backbone.buffers()}
    loss, g = step(model, xg, yg)
    assert sorted(g) == sorted(names) and all(p.grad is None for p in model.backbone.parameters())
    for k, b in model.named_buffers():
        if id(b) in inside:
            assert torch.equal(b, before[k]), k
    ref_l, got_l = abs(float(le) - float(l64)) / abs(float(l64)), abs(loss.item() - float(l64)) / abs(float(l64))
    assert got_l <= 3.0 * ref_l + 1e-3
    gnorm = float(torch.sqrt(sum((t ** 2).sum() for t in g64.values())))
    bad, worst = [], (0.0, None)
    for k in names:
        d = float((g[k].double().cpu() - g64[k]).norm())
        bound = 6.0 * float((ge[k] - g64[k]).norm()) + 1e-3 * float(g64[k].norm()) + 1e-4 * gnorm
        worst = max(worst, (d / bound, k))
        if d > bound:
            bad.append((k, d, bound))
    print(f"bf16io worst gradient {worst[0]:.3f} of its bound ({worst[1]}), loss err {got_l:.3e} (reference {ref_l:.3e})")
    assert not bad, bad[:8]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def test_forward_loss_options_under_a_frozen_backbone(data):
    """tests/test_gpu_loss_options_model.py::test_gradients_fused_against_logits_path's assertions, with the
    backbone frozen: the fused weighted / smoothed loss against the logits path of the same criterion."""
    _, _, xg, yg = data
    model = freeze(build().to(DEV)).train()
    w = (torch.rand(10, generator=torch.Generator().manual_seed(5)) * 3 + 0.05).to(DEV)
    crit = nn.CrossEntropyLoss(weight=w, label_smoothing=0.1).to(DEV)
    plain = nn.CrossEntropyLoss()

    def logits_path(c):
        model.zero_grad(set_to_none=True)
        loss = c(model(xg), yg)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), named_grads(model)

    _, gf = step(model, xg, yg)
    _, gl = logits_path(plain)
    lf, wf = step(model, xg, yg, weight=w, label_smoothing=0.1)
    ll, wl = logits_path(crit)
    assert wf.keys() == wl.keys() == gf.keys() and not any(k.startswith("backbone.") for k in wf)
    assert abs(lf.item() - ll.item()) <= 1e-5 * abs(ll.item())
    plain_rel = {k: rel(gf[k], gl[k]) for k in gf}
    w_rel = {k: rel(wf[k], wl[k]) for k in wf}
    worst = max(plain_rel.values())
    print(f"plain worst {worst:.3e}, weighted worst {max(w_rel.values()):.3e}, head "
          f"{w_rel['outc.conv.3.weight']:.3e} {w_rel['outc.conv.3.bias']:.3e}")
    assert w_rel["outc.conv.3.weight"] < 1e-4 and w_rel["outc.conv.3.bias"] < 1e-4
    for k, v in w_rel.items():
        assert v <= 2 * worst, (k, v, worst)


def test_unet_inc_and_down1_frozen():
    x, y = synthetic_batch(2, 32, 64, 4, seed=112)
    ctor = lambda: UNet(4)  # noqa: E731
    cpu = build(ctor, seed=12)
    model = freeze(build(ctor, seed=12).to(DEV), ["inc", "down1"]).train()
    before = buffers(model)
    inside = {id(b) for mod in (model.inc, model.down1) for b in mod.buffers()}
    loss, g, z, pools = hip_step(model, x.to(DEV), y.to(DEV))
    state = segref.canonical_state(cpu.state_dict())
    names = [k for k in segref.trainable_names(state) if not k.startswith(("inc.", "down1."))]
    assert sorted(g) == sorted(names)
    loss64, _ = three_part_check(unet_forward_inc_down1_frozen, names, cpu, x, y, g, z, pools)
    assert abs(loss.item() - loss64) <= 1e-3 * abs(loss64)
    for k, b in model.named_buffers():
        assert torch.equal(b, before[k]) is (id(b) in inside), k


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


def test_data_parallel_world1(pg, data):
    from seg_amd.ddp import DataParallel
    _, _, xg, yg = data
    plain = freeze(build().to(DEV)).train()
    wrapped = DataParallel(freeze(build().to(DEV)).train(), bucket_cap_mb=1.0)
    wrapped.train()  # recurses into the module, whose train() keeps the freeze
    assert not any(m.training for m in wrapped.module.backbone.modules() if isinstance(m, nn.BatchNorm2d))
    _, gp = step(plain, xg, yg)
    _, gw = step(wrapped, xg, yg)
    assert gp.keys() == gw.keys() and 0 < len(gp) < 194
    for k in gp:
        assert torch.equal(gp[k], gw[k]), k
    gen, slots = wrapped.generation, len(wrapped._slot)
    unfreeze(plain)
    unfreeze(wrapped)
    _, gp = step(plain, xg, yg)
    _, gw = step(wrapped, xg, yg)
    assert wrapped.generation == gen + 1 and len(wrapped._slot) > slots  # the buckets were planned anew
    assert gp.keys() == gw.keys() and len(gp) == 194
    for k in gp:
        assert torch.equal(gp[k], gw[k]), k
