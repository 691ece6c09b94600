"""CPU: seg_amd.freeze / unfreeze / frozen_modules, the train() override that keeps a freeze, traceable() carrying
it over, and the training loop honouring it (the CPU composition runs the modules themselves)."""
import json
import os

import pytest
import torch
from torch import nn

import seg_amd
from seg_amd import MobileNetV2UNet, UNet, deterministic_init, freeze, frozen_modules, synthetic_batch, unfreeze

BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def bns(mod):
    return [m for m in mod.modules() if isinstance(m, nn.BatchNorm2d)]


def backbone_ids(model):
    return {id(t) for t in list(model.backbone.parameters()) + list(model.backbone.buffers())}


def split_state(model):
    """(backbone, rest): name -> clone of every parameter and BatchNorm buffer, aliases (down1..5) once."""
    inside = backbone_ids(model)
    back, rest, seen = {}, {}, set()
    for k, t in list(model.named_parameters()) + list(model.named_buffers()):
        if id(t) in seen:
            continue
        seen.add(id(t))
        (back if id(t) in inside else rest)[k] = t.detach().clone()
    return back, rest


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_freeze_backbone_flags_and_state_dict(golden_dir):
    m = MobileNetV2UNet(10)
    assert freeze(m) is m
    inside = {id(p) for p in m.backbone.parameters()}
    for p in m.parameters():
        assert p.requires_grad is (id(p) not in inside)
    frozen_bn = {id(b) for b in bns(m.backbone)}
    for prepare in (lambda: m.train(), lambda: (m.eval(), m.train())):
        prepare()
        assert m.training
        for b in bns(m):
            assert b.training is (id(b) not in frozen_bn)
    m.eval()
    assert not any(b.training for b in bns(m))
    m.train()
    with open(os.path.join(golden_dir, "state_dict_keys.json")) as f:
        ref = json.load(f)["MobileNetV2UNet"]
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref
    assert [n for n, _ in m.named_children()] == [n for n, _ in MobileNetV2UNet(10).named_children()]
    assert frozen_modules(m) == {"backbone": {"params": True, "bn_stats": True}}


def test_unfreeze_restores_everything():
    m = MobileNetV2UNet(10).train()
    freeze(m)
    unfreeze(m)
    assert all(p.requires_grad for p in m.parameters())
    assert all(b.training for b in bns(m))
    assert frozen_modules(m) == {}
    m.eval()
    m.train()
    assert all(b.training for b in bns(m))
    # parts: BatchNorm statistics only, and an overlapping entry that stays
    freeze(m, "backbone", params=False)
    assert all(p.requires_grad for p in m.parameters()) and not any(b.training for b in bns(m.backbone))
    freeze(m, m.down1)
    unfreeze(m, "backbone")
    assert frozen_modules(m) == {"down1": {"params": True, "bn_stats": True}}
    assert not any(p.requires_grad for p in m.down1.parameters())
    assert all(not b.training for b in bns(m.down1)) and all(b.training for b in bns(m.down2))
    with pytest.raises(AttributeError):
        freeze(m, "no_such_block")


def test_unet_parts():
    u = UNet(4).train()
    freeze(u, ["inc", "down1"])
    inside = {id(p) for mod in (u.inc, u.down1) for p in mod.parameters()}
    frozen_bn = {id(b) for mod in (u.inc, u.down1) for b in bns(mod)}
    u.train()
    assert all(p.requires_grad is (id(p) not in inside) for p in u.parameters())
    assert all(b.training is (id(b) not in frozen_bn) for b in bns(u))
    assert list(frozen_modules(u)) == ["inc", "down1"]


def test_traceable_carries_the_freeze():
    m = MobileNetV2UNet(10).train()
    freeze(m)
    m.outc.conv[3].bias.requires_grad_(False)
    m.up2.conv.conv[1].eval()
    t = seg_amd.traceable(m)
    assert {k: p.requires_grad for k, p in t.named_parameters()} == {k: p.requires_grad for k, p in m.named_parameters()}
    assert {k: mod.training for k, mod in t.named_modules()} == {k: mod.training for k, mod in m.named_modules()}
    assert frozen_modules(t) == frozen_modules(m)
    t.train()  # the twin keeps the freeze as the model does
    assert not any(b.training for b in bns(t.backbone)) and t.up2.conv.conv[1].training


@pytest.fixture(scope="module")
def batches():
    return [synthetic_batch(2, 64, 64, 10, seed=300 + i) for i in range(2)]


def test_train_one_epoch_leaves_a_frozen_backbone_alone(batches):
    m = deterministic_init(MobileNetV2UNet(10), seed=3, random_running_stats=True)
    freeze(m)
    back0, rest0 = split_state(m)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    seg_amd.train_one_epoch(m, batches, nn.CrossEntropyLoss(), opt, torch.device("cpu"), progress=False)
    back1, rest1 = split_state(m)
    assert same(back0, back1)  # bitwise: parameters, running statistics, num_batches_tracked
    assert all(p.grad is None for p in m.backbone.parameters())
    for k in rest0:  # every decoder parameter and BatchNorm buffer moved
        assert not torch.equal(rest0[k], rest1[k]), k
    assert any(k.endswith(BN_BUFFERS) for k in rest0)


def test_train_model_unfreezes_after_freeze_epochs(batches, tmp_path, capsys):
    m = deterministic_init(MobileNetV2UNet(10), seed=3, random_running_stats=True)
    back0, _ = split_state(m)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    pattern = str(tmp_path / "epoch_{epoch}.pth")
    seg_amd.train_model(m, batches, nn.CrossEntropyLoss(), opt, torch.device("cpu"), epochs=2,
                        checkpoint_pattern=pattern, progress=False, freeze="backbone", freeze_epochs=1)
    after1 = torch.load(pattern.format(epoch=1))
    assert all(torch.equal(after1[k], v) for k, v in back0.items())
    back2, _ = split_state(m)
    used = [k for k in back0 if not k.startswith("backbone.classifier")]
    assert all(not torch.equal(back0[k], back2[k]) for k in used)
    assert frozen_modules(m) == {} and all(p.requires_grad for p in m.parameters())
    lines = capsys.readouterr().out.splitlines()
    assert [l.split(":")[0] for l in lines if "rozen" in l] == ["Frozen for 1 epoch(s)", "Unfrozen before epoch 2"]


@pytest.mark.parametrize("name", ["seg_bn_frozen_backward", "seg_bn_frozen_backward_bf16io"])
def test_frozen_backward_rejects_bad_arguments_without_a_launch(name):
    """hipErrorInvalidValue (1) before any launch, so no GPU is needed: C, the row strides, missing operands;
    M < 1 is a no-op."""
    from seg_amd import _lib
    from seg_amd.build import build
    build()
    fn = getattr(_lib.lib(), name)
    X = 0x1000  # never dereferenced: every call below returns before a launch
    good = dict(da=X, ldda=8, y=X, ldy=8, M=16, C=8, scale=X, shift=X, rm=X, rv=X, eps=1e-5, act=2, dgamma=X, dbeta=X,
                work=X, dy=X, lddy=8, stream=None)
    for bad in (dict(C=6), dict(C=0), dict(ldda=6), dict(ldy=10), dict(lddy=7), dict(M=1 << 31), dict(da=None),
                dict(y=None), dict(scale=None), dict(shift=None), dict(work=None), dict(rm=None), dict(rv=None)):
        assert fn(*{**good, **bad}.values()) == 1, bad
    assert fn(*{**good, "M": 0}.values()) == 0
    assert fn(*{**good, "M": 0, "da": None, "y": None}.values()) == 0
    assert fn(*{**good, "dgamma": None, "dbeta": None, "dy": None, "work": None}.values()) == 0  # nothing asked for


def test_train_model_without_freeze_prints_what_it_did(batches, capsys):
    m = deterministic_init(MobileNetV2UNet(10), seed=3)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    seg_amd.train_model(m, batches[:1], nn.CrossEntropyLoss(), opt, torch.device("cpu"), epochs=1,
                        checkpoint_pattern=None, progress=False)
    out = capsys.readouterr().out
    assert "rozen" not in out and out.splitlines()[0].startswith("  Training Loss:")
