"""CPU: the host side of seg_amd.AdamW, grad_norm / clip_grad_norm_, decay_groups and train_one_epoch's
max_grad_norm -- the SegAdamWTensor table layout (include/segamd.h), refusals (no silent fallback), the
parameter groups, the delegation of CPU tensors to torch's clip, and the new entry points' argument validation
(before any launch: no GPU needed).  The kernels themselves: tests/test_gpu_adamw.py."""
import ctypes

import pytest
import torch
from torch import nn

import seg_amd
from seg_amd import AdamW, MobileNetV2UNet, UNet, clip_grad_norm_, decay_groups, deterministic_init, synthetic_batch
from seg_amd.optim import _pack_w
from seg_amd.train import compute_loss, train_one_epoch


class SegAdamWTensor(ctypes.Structure):  # include/segamd.h
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("n", ctypes.c_long), ("step_size", ctypes.c_float), ("bc2_sqrt", ctypes.c_float),
                ("decay", ctypes.c_float), ("pad", ctypes.c_float)]


def test_table_layout():
    rows = [(0x1000, 0x2000, 0x3000, 0x4000, 7, -1.5e-3, 0.031622776, 0.9999985, 0.0),
            (16, 32, 48, 64, 1 << 33, -2.0, 1.0, 1.0, 0.0)]
    t = _pack_w(rows)
    assert t.dtype == torch.int64 and t.shape == (2, 7) and t.is_contiguous()
    assert ctypes.sizeof(SegAdamWTensor) == 7 * 8 == 56
    arr = (SegAdamWTensor * 2).from_buffer_copy(t.numpy().tobytes())
    for r, e in zip(rows, arr):
        assert (e.p, e.g, e.m, e.v, e.n) == r[:5]
        for got, want in zip((e.step_size, e.bc2_sqrt, e.decay, e.pad), r[5:]):
            assert got == pytest.approx(want, rel=1e-7)


def test_refuses_unsupported():
    p = torch.nn.Parameter(torch.randn(4))
    p.grad = torch.randn(4)
    with pytest.raises(NotImplementedError):
        AdamW([p], lr=1e-3).step()  # CPU tensors: the HIP step only
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}):
        with pytest.raises(NotImplementedError):
            AdamW([p], lr=1e-3, **kw).step()
    q = torch.nn.Parameter(torch.randn(4))  # no gradient: skipped, nothing to do
    opt = AdamW([q], lr=1e-3)
    opt.step()
    assert len(opt.state) == 0
    assert issubclass(AdamW, torch.optim.AdamW) and opt.param_groups[0]["weight_decay"] == 1e-2


def test_grad_norm_without_gradients():
    q = torch.nn.Parameter(torch.randn(4))
    assert seg_amd.grad_norm([q]).tolist() == [0.0, 1.0, 0.0]
    assert seg_amd.grad_norm([], 1.0).tolist() == [0.0, 1.0, 0.0]
    q.grad = torch.randn(4)
    with pytest.raises(NotImplementedError):
        seg_amd.grad_norm([q])  # CPU gradients: the HIP reduction only


def test_decay_groups():
    model = MobileNetV2UNet(10)
    groups = decay_groups(model, 1e-2)
    assert [g["weight_decay"] for g in groups] == [1e-2, 0.0]
    ids = [id(p) for g in groups for p in g["params"]]
    trainable = [id(p) for p in model.parameters() if p.requires_grad]
    assert len(ids) == len(set(ids)) and sorted(ids) == sorted(trainable)
    assert all(p.ndim > 1 for p in groups[0]["params"])
    decayed = {id(p) for p in groups[0]["params"]}
    assert not any(id(p) in decayed for p in model.parameters() if p.ndim == 1)
    bn = {id(p) for m in model.modules() if isinstance(m, nn.BatchNorm2d) for p in m.parameters()}
    assert bn and not bn & decayed
    conv_w = {id(m.weight) for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
    assert conv_w == decayed
    seg_amd.freeze(model)
    groups = decay_groups(model, 1e-2)
    ids = {id(p) for g in groups for p in g["params"]}
    assert ids and not ids & {id(p) for p in model.backbone.parameters()}
    assert ids == {id(p) for n, p in model.named_parameters() if not n.startswith("backbone.")}
    torch.optim.AdamW(groups, lr=1e-3)  # the groups are what an optimizer takes


def test_clip_grad_norm_cpu_is_torchs():
    g = torch.Generator().manual_seed(3)
    a = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 7), (3,), (11,))]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    for i, (p, q) in enumerate(zip(a, b)):
        if i != 1:  # one parameter without a gradient
            p.grad = torch.randn(p.shape, generator=g)
            q.grad = p.grad.clone()
    n1 = clip_grad_norm_(a, 0.5)
    n2 = torch.nn.utils.clip_grad_norm_(b, 0.5)
    assert torch.equal(n1, n2) and float(n1) > 0.5
    assert a[1].grad is None and all(torch.equal(p.grad, q.grad) for p, q in zip(a, b) if p.grad is not None)
    with pytest.raises(ValueError):
        clip_grad_norm_(a, 0.0)


def test_train_one_epoch_max_grad_norm_cpu():
    """A CPU model and torch.optim.AdamW: the loop clips with clip_grad_norm_ (torch's, on CPU tensors) after the
    backward and before the step -- bitwise a hand-written loop."""
    batches = [synthetic_batch(2, 32, 64, 4, seed=s) for s in (1, 2)]
    crit = nn.CrossEntropyLoss()
    ours, ref = (deterministic_init(UNet(4, 8), seed=1).train() for _ in range(2))
    o1 = torch.optim.AdamW(ours.parameters(), lr=1e-3, weight_decay=1e-2)
    o2 = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-2)
    train_one_epoch(ours, batches, crit, o1, "cpu", progress=False, max_grad_norm=0.5)
    norms = []
    for x, y in batches:
        o2.zero_grad()
        compute_loss(ref, crit, x, y).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)))
        o2.step()
    assert min(norms) > 0.5, norms  # the clip was active
    for (k, a), b in zip(ours.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), k


def test_argument_validation_without_gpu():
    from seg_amd import _lib
    from seg_amd.build import build
    build()
    lib = _lib.lib()
    # hipErrorInvalidValue == 1 for chunk < 1 or nchunks < 0, hipSuccess for nothing to do: before any launch
    assert lib.seg_adamw_step(None, None, 4, 0, 0.1, 0.999, 0.001, 1e-8, None, None, None) == 1
    assert lib.seg_grad_sumsq(None, None, 4, 0, 1.0, None, None, None) == 1
    assert lib.seg_grad_scale(None, None, 4, 0, None, None) == 1
    assert lib.seg_adamw_step(None, None, -1, 4096, 0.1, 0.999, 0.001, 1e-8, None, None, None) == 1
    assert lib.seg_adamw_step(None, None, 0, 4096, 0.1, 0.999, 0.001, 1e-8, None, None, None) == 0
    assert lib.seg_grad_sumsq(None, None, 0, 4096, 1.0, None, None, None) == 0
    assert lib.seg_grad_scale(None, None, 0, 4096, None, None) == 0
    assert _lib.query("seg_grad_norm_workspace_floats", 1077) >= 1077
    assert _lib.query("seg_grad_norm_workspace_floats", 0) == 0
