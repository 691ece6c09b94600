"""GPU: the fine-tuning recipe through the training loop -- MobileNetV2UNet(10) at 2x3x64x64,
seg_amd.AdamW(decay_groups(model, 1e-2)) and train_one_epoch(..., max_grad_norm=...).

The reference of a step is torch's: the same engine gradients (a twin model: the engine's gradients are bitwise
reproducible), torch.nn.utils.clip_grad_norm_ on them, then torch.optim.AdamW on the same groups.  One step only:
after it the two runs' gradients differ and Adam's normalisation amplifies the difference.  Parameters agree to
rtol 2e-5 (the clip coefficient's 1e-5 plus rounding; tests/test_gpu_adamw.py) and atol 1e-7.
"""
import pytest
import torch
from torch import nn

from seg_amd import AdamW, MobileNetV2UNet, decay_groups, freeze, grad_norm, train_model, train_one_epoch
from seg_amd.detinit import deterministic_init, synthetic_batch
from seg_amd.train import compute_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 1e-3


def build(frozen=False):
    m = deterministic_init(MobileNetV2UNet(10), seed=11).to(DEV)
    if frozen:
        freeze(m)
    return m.train()


@pytest.fixture(scope="module")
def batch():
    return synthetic_batch(2, 64, 64, 10, seed=111)


def torch_step(model, x, y, max_norm_of):
    """One reference step on `model`; returns (the gradients before the clip, their float64 norm, max_norm)."""
    crit = nn.CrossEntropyLoss()
    opt = torch.optim.AdamW(decay_groups(model, 1e-2), lr=LR)
    opt.zero_grad()
    compute_loss(model, crit, x.to(DEV), y.to(DEV)).backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    max_norm = max_norm_of(norm)
    torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], max_norm)
    opt.step()
    torch.cuda.synchronize()
    return grads, norm, max_norm


@pytest.mark.parametrize("frozen", [False, True])
def test_one_clipped_step_matches_torch(batch, frozen):
    x, y = batch
    ref, ours = build(frozen), build(frozen)
    start = {k: p.detach().clone() for k, p in ours.named_parameters()}
    grads, norm, max_norm = torch_step(ref, x, y, lambda n: n / 2)  # half the measured norm: the clip is active
    opt = AdamW(decay_groups(ours, 1e-2), lr=LR)
    train_one_epoch(ours, [(x, y)], nn.CrossEntropyLoss(), opt, DEV, progress=False, max_grad_norm=max_norm)
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in ours.named_parameters() if p.grad is not None}
    assert got.keys() == grads.keys()
    for k in grads:
        assert torch.equal(got[k], grads[k]), k  # the same engine gradients, and .grad stays unclipped
    out = grad_norm([p for g in opt.param_groups for p in g["params"]], max_norm)
    print(f"frozen={frozen}: norm {float(out[0]):.6g} (float64 {norm:.6g}), coefficient {float(out[1]):.6g}")
    assert abs(float(out[0]) - norm) <= 1e-5 * norm and 0.49 < float(out[1]) < 0.51
    moved = 0
    for (k, a), b in zip(ours.named_parameters(), ref.parameters()):
        if frozen and k.startswith("backbone."):
            assert a.grad is None and torch.equal(a, start[k]), k  # bitwise where it was
            continue
        torch.testing.assert_close(a, b, rtol=2e-5, atol=1e-7, msg=lambda m: f"{k}: {m}")
        moved += int(not torch.equal(a, start[k]))
    assert moved > len(grads) // 2  # (a conv bias in front of a BatchNorm has a zero gradient and no decay)
    if frozen:  # the backbone is not in the norm: the decoder's gradients alone give it
        assert not any(k.startswith("backbone.") for k in grads)
        decoder = [p for k, p in ours.named_parameters() if not k.startswith("backbone.")]
        assert torch.equal(grad_norm(decoder)[0], out[0])
    for (k, a), b in zip(ours.named_buffers(), ref.buffers()):
        assert torch.equal(a, b), k


def test_unclipped_step_is_the_plain_step(batch):
    """max_grad_norm far above the norm: the coefficient is exactly 1 and the step is bitwise the one without."""
    x, y = batch
    a, b = build(), build()
    oa, ob = AdamW(decay_groups(a, 1e-2), lr=LR), AdamW(decay_groups(b, 1e-2), lr=LR)
    train_one_epoch(a, [(x, y)], nn.CrossEntropyLoss(), oa, DEV, progress=False, max_grad_norm=1e6)
    train_one_epoch(b, [(x, y)], nn.CrossEntropyLoss(), ob, DEV, progress=False)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k


def test_out_of_range_label_skips_the_clipped_step(batch):
    x, y = batch
    model = build()
    opt = AdamW(decay_groups(model, 1e-2), lr=LR)
    crit = nn.CrossEntropyLoss()
    train_one_epoch(model, [(x, y)], crit, opt, DEV, progress=False, max_grad_norm=1.0)
    torch.cuda.synchronize()
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    state = [{k: v.clone() for k, v in opt.state[p].items()} for g in opt.param_groups for p in g["params"]]
    bad = y.clone()
    bad[0, 0, 0] = 10
    with pytest.raises(IndexError):
        train_one_epoch(model, [(x, bad)], crit, opt, DEV, progress=False, max_grad_norm=1.0)
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        assert torch.equal(p, params[k]), k
    now = [opt.state[p] for g in opt.param_groups for p in g["params"]]
    assert len(now) == len(state)
    for s0, s1 in zip(state, now):
        assert s0.keys() == s1.keys()
        assert all(torch.equal(s0[k], s1[k]) for k in s0)  # exp_avg, exp_avg_sq and step (== 1)


def test_train_model_without_max_grad_norm_is_unchanged(batch):
    x, y = batch
    x2, y2 = synthetic_batch(2, 64, 64, 10, seed=112)
    a, b = build(), build()
    oa, ob = AdamW(decay_groups(a, 1e-2), lr=LR), AdamW(decay_groups(b, 1e-2), lr=LR)
    kw = dict(epochs=1, checkpoint_pattern=None, progress=False)
    train_model(a, [(x, y), (x2, y2)], nn.CrossEntropyLoss(), oa, DEV, max_grad_norm=None, **kw)
    train_model(b, [(x, y), (x2, y2)], nn.CrossEntropyLoss(), ob, DEV, **kw)
    for (k, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(p, q), k
    for ga, gb in zip(oa.param_groups, ob.param_groups):
        for p, q in zip(ga["params"], gb["params"]):
            assert oa.state[p].keys() == ob.state[q].keys()
            assert all(torch.equal(v, ob.state[q][k]) for k, v in oa.state[p].items())
