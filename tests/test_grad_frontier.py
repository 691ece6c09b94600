"""CPU: engine.grad_frontier (what the backward owes each op once parts of a model are frozen) and
engine.plan_signature (what makes a recorded plan stale), on programs built without the library."""
import pytest
from torch import nn

from seg_amd import MobileNetV2UNet, UNet, engine, freeze
from seg_amd.engine import ConvOp, PoolOp, UpsampleOp


@pytest.fixture()
def mnv2():
    m = MobileNetV2UNet(10)
    return m, (lambda: engine.build_mobilenet_unet(m, 2, 64, 64))


def today(prog):
    """The backward before freezing existed: parameter gradients for every op with parameters, a data gradient
    for every op but the one reading the image."""
    return [(bool(op.params()), not getattr(op, "first", False)) for op in prog.ops]


def op_index(prog, conv):
    return next(k for k, op in enumerate(prog.ops) if isinstance(op, ConvOp) and op.conv is conv)


def test_nothing_frozen_is_todays_backward(mnv2):
    m, build = mnv2
    prog = build()
    assert len(prog.ops) == 66 and sum(isinstance(op, ConvOp) and op.lazy for op in prog.ops) == 35
    assert engine.grad_frontier(prog) == today(prog)
    u = UNet(4)
    prog = engine.build_unet(u, 2, 32, 64)
    assert engine.grad_frontier(prog) == today(prog)


@pytest.mark.parametrize("shape", [(2, 64, 64), (1, 256, 512)])
def test_backbone_frozen(mnv2, shape):
    m, _ = mnv2
    freeze(m)
    prog = engine.build_mobilenet_unet(m, *shape)
    gf = engine.grad_frontier(prog)
    assert isinstance(prog.ops[52], UpsampleOp) and prog.ops[53].conv is m.up1.conv.conv[0]
    assert (prog.ops[53].cin, prog.ops[53].cout) == (1344, 256)
    assert gf[:53] == [(False, False)] * 53          # the encoder and up1's upsample: nothing
    assert gf[53] == (True, False)                   # up1's first conv: parameter gradients only
    assert gf[54:] == today(prog)[54:]               # the rest of the decoder: as today


def test_first_seven_feature_blocks_frozen(mnv2):
    m, build = mnv2
    feats = m.backbone.features
    freeze(m, [feats[i] for i in range(7)])
    prog = build()
    gf = engine.grad_frontier(prog)
    first = op_index(prog, feats[7].conv[0][0])      # features[7]'s expand conv
    assert gf[:first] == [(False, False)] * first
    assert gf[first] == (True, False)                # its input comes from the frozen part
    assert gf[first + 1:] == today(prog)[first + 1:]
    # the skips x1..x3 (features[1], [3], [6]) need no gradient, x4 (features[10]) does: their producers
    for i, want in ((1, False), (3, False), (6, False), (10, True)):
        k = op_index(prog, feats[i].conv[-2])        # the block's project conv writes the skip slice
        assert gf[k][0] is want and prog.ops[k].out.buf.startswith("cat")
    ups = [k for k, op in enumerate(prog.ops) if isinstance(op, UpsampleOp)]
    assert all(gf[k] == (False, True) for k in ups)


def test_only_batchnorm_affine_frozen(mnv2):
    m, build = mnv2
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.requires_grad_(False)
    prog = build()
    assert engine.grad_frontier(prog) == today(prog)  # the convs still train: every gradient as today


def test_unet_inc_and_down1_frozen():
    u = UNet(4)
    freeze(u, ["inc", "down1"])
    prog = engine.build_unet(u, 2, 32, 64)
    gf = engine.grad_frontier(prog)
    assert isinstance(prog.ops[2], PoolOp) and isinstance(prog.ops[5], PoolOp)
    assert gf[:6] == [(False, False)] * 6
    assert gf[6] == (True, False)
    assert gf[7:] == today(prog)[7:]


def test_plan_signature_sees_one_flag(mnv2):
    m, build = mnv2
    prog = build()
    base = engine.plan_signature(prog)
    assert engine.plan_signature(prog) == base
    bn = m.backbone.features[3].conv[1][1]
    bn.eval()
    flipped = engine.plan_signature(prog)
    assert flipped != base
    bn.train()
    assert engine.plan_signature(prog) == base
    m.up3.conv.conv[0].bias.requires_grad_(False)
    assert engine.plan_signature(prog) not in (base, flipped)
