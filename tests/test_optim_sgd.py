"""CPU: the host side of seg_amd.SGD -- the table it packs for seg_sgd_step (the SegAdamWTensor record of
include/segamd.h, filled as the header says for SGD), its refusals (no silent fallback), torch's own constructor
errors, the entry point's argument validation (before any launch: no GPU needed) -- and the scheduler arguments of
train_one_epoch / train_model on a CPU model.  The kernel itself: tests/test_gpu_sgd.py."""
import ctypes

import pytest
import torch
from torch import nn

import seg_amd
from seg_amd import SGD, PolyLR, UNet, deterministic_init, synthetic_batch
from seg_amd.optim import _pack_w
from seg_amd.train import train_model, train_one_epoch


class SegSgdTensor(ctypes.Structure):  # include/segamd.h: SegAdamWTensor as seg_sgd_step reads it
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("buf", ctypes.c_void_p), ("unused", ctypes.c_void_p),
                ("n", ctypes.c_long), ("step_size", ctypes.c_float), ("bc2_sqrt", ctypes.c_float),
                ("decay", ctypes.c_float), ("seed", ctypes.c_float)]


def test_table_layout():
    # the rows SGD.step() builds: (p, g, momentum_buffer or 0, 0, n, 0, 1, 1, seed)
    rows = [(0x1000, 0x2000, 0x3000, 0, 7, 0.0, 1.0, 1.0, 1.0), (16, 32, 0, 0, 1 << 33, 0.0, 1.0, 1.0, 0.0)]
    t = _pack_w(rows)
    assert t.dtype == torch.int64 and t.shape == (2, 7) and t.is_contiguous()
    assert ctypes.sizeof(SegSgdTensor) == 7 * 8 == 56
    assert SegSgdTensor.buf.offset == 16 and SegSgdTensor.n.offset == 32 and SegSgdTensor.seed.offset == 52
    arr = (SegSgdTensor * 2).from_buffer_copy(t.numpy().tobytes())
    for r, e in zip(rows, arr):
        assert (e.p or 0, e.g or 0, e.buf or 0, e.unused or 0, e.n) == r[:5]
        assert (e.step_size, e.bc2_sqrt, e.decay, e.seed) == r[5:]


def test_refuses_unsupported():
    p = torch.nn.Parameter(torch.randn(4))
    p.grad = torch.randn(4)
    for kw in ({}, {"momentum": 0.9}, {"momentum": 0.9, "nesterov": True, "weight_decay": 5e-4}):
        opt = SGD([p], lr=1e-2, **kw)
        with pytest.raises(NotImplementedError):
            opt.step()  # CPU tensors: the HIP step only
        assert len(opt.state) == 0  # and nothing was created on the way
    for kw in ({"maximize": True}, {"differentiable": True}):
        with pytest.raises(NotImplementedError):
            SGD([p], lr=1e-2, **kw).step()
    h = torch.nn.Parameter(torch.randn(4, dtype=torch.float64))
    h.grad = torch.randn(4, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        SGD([h], lr=1e-2).step()
    q = torch.nn.Parameter(torch.randn(4))  # no gradient: absent from the table, nothing to do
    opt = SGD([q], lr=1e-2, momentum=0.9)
    opt.step()
    assert len(opt.state) == 0 and opt.state_dict()["state"] == {}
    opt.undo_step_count()  # nothing to take back
    with pytest.raises(ValueError):
        opt.step(skip_if_nonzero=torch.zeros(1))  # a CPU flag
    with pytest.raises(NotImplementedError):  # pinned by tests/test_optim.py: Adam keeps refusing the L2 form
        seg_amd.Adam([p], lr=1e-3, weight_decay=1e-2).step()


def test_constructor_is_torchs():
    p = torch.nn.Parameter(torch.randn(4))
    assert issubclass(SGD, torch.optim.SGD)
    ours, ref = SGD([p], lr=1e-2, momentum=0.9, nesterov=True, weight_decay=5e-4), \
        torch.optim.SGD([p], lr=1e-2, momentum=0.9, nesterov=True, weight_decay=5e-4)
    assert ours.param_groups[0].keys() == ref.param_groups[0].keys()
    assert {k: v for k, v in ours.param_groups[0].items() if k != "params"} == \
        {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    d = SGD([p]).defaults
    assert (d["lr"], d["momentum"], d["dampening"], d["weight_decay"], d["nesterov"]) == (1e-3, 0, 0, 0, False)
    for kw in ({"nesterov": True}, {"nesterov": True, "momentum": 0.9, "dampening": 0.1}, {"lr": -1.0},
               {"momentum": -0.5}, {"weight_decay": -1e-4}):
        with pytest.raises(ValueError):  # torch's own errors stay torch's
            SGD([p], **kw)
        with pytest.raises(ValueError):
            torch.optim.SGD([p], **kw)
    ours.load_state_dict(ref.state_dict())  # an empty state moves both ways
    ref.load_state_dict(ours.state_dict())


def test_argument_validation_without_gpu():
    from seg_amd import _lib
    from seg_amd.build import build
    build()
    lib = _lib.lib()
    # hipErrorInvalidValue == 1 for chunk < 1 or nchunks < 0, hipSuccess for nothing to do: before any launch
    assert lib.seg_sgd_step(None, None, 4, 0, 1e-2, 0.9, 1.0, 5e-4, 1, None, None, None) == 1
    assert lib.seg_sgd_step(None, None, -1, 4096, 1e-2, 0.9, 1.0, 5e-4, 1, None, None, None) == 1
    assert lib.seg_sgd_step(None, None, 0, 4096, 1e-2, 0.9, 1.0, 5e-4, 1, None, None, None) == 0


# ---------------------------------------------------------------- the scheduler arguments of the loop (CPU model)

def _cpu_run(seed=1):
    model = deterministic_init(UNet(4, 8), seed=seed).train()
    return model, torch.optim.SGD(model.parameters(), lr=1e-2, momentum=0.9)


@pytest.fixture(scope="module")
def batches():
    return [synthetic_batch(2, 32, 64, 4, seed=s) for s in (1, 2, 3)]


def test_train_one_epoch_steps_the_scheduler_per_batch(batches):
    model, opt = _cpu_run()
    sched = PolyLR(opt, total_iters=6, warmup_iters=2)
    lrs = []

    class Spy(list):  # the learning rate each batch is stepped with: read when the batch is fetched
        def __iter__(self):
            for b in batches:
                lrs.append(opt.param_groups[0]["lr"])
                yield b

    train_one_epoch(model, Spy(batches), nn.CrossEntropyLoss(), opt, "cpu", progress=False, scheduler=sched)
    assert sched.last_epoch == len(batches) == 3
    assert lrs == [sched._lr_at(1e-2, t) for t in range(3)]
    assert opt.param_groups[0]["lr"] == sched._lr_at(1e-2, 3)


def test_train_model_scheduler_intervals(batches):
    crit = nn.CrossEntropyLoss()
    kw = dict(epochs=2, checkpoint_pattern=None, progress=False)
    model, opt = _cpu_run()
    sched = PolyLR(opt, total_iters=6)
    train_model(model, batches, crit, opt, "cpu", scheduler=sched, **kw)  # "step" is the default
    assert sched.last_epoch == 2 * len(batches)
    model, opt = _cpu_run()
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    train_model(model, batches, crit, opt, "cpu", scheduler=sched, scheduler_interval="epoch", **kw)
    assert sched.last_epoch == 2 and opt.param_groups[0]["lr"] == pytest.approx(1e-2 * 0.25)
    model, opt = _cpu_run()
    start = [p.detach().clone() for p in model.parameters()]
    for bad in ("batch", "", None):
        with pytest.raises(ValueError):
            train_model(model, batches, crit, opt, "cpu", scheduler=PolyLR(opt, 6), scheduler_interval=bad, **kw)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), start))  # refused before anything ran


def test_scheduler_none_is_the_unchanged_call(batches):
    crit = nn.CrossEntropyLoss()
    kw = dict(epochs=2, checkpoint_pattern=None, progress=False)
    (a, oa), (b, ob) = _cpu_run(), _cpu_run()
    train_model(a, batches, crit, oa, "cpu", scheduler=None, **kw)
    train_model(b, batches, crit, ob, "cpu", **kw)
    for (k, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(p, q), k
    (c, oc), (d, od) = _cpu_run(), _cpu_run()
    train_one_epoch(c, batches, crit, oc, "cpu", progress=False, scheduler=None)
    train_one_epoch(d, batches, crit, od, "cpu", progress=False)
    for (k, p), q in zip(c.state_dict().items(), d.state_dict().values()):
        assert torch.equal(p, q), k
    assert not torch.equal(next(iter(c.parameters())), next(iter(deterministic_init(UNet(4, 8), seed=1).parameters())))
