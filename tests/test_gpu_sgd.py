"""GPU: seg_amd.SGD (seg_sgd_step of csrc/adam.hip) against torch.optim.SGD in float64, and its bitwise properties.

Shapes, gradients and groups: tests/test_gpu_adamw.py's -- 4095 / 4096 / 4097 elements on the chunk edge, 1- and
3-element tensors, half-zero gradients in tensor 1, gradients scaled by 10^-(3 (i % 4)), a last tensor without a
gradient; ps[:4] with the configuration's weight decay, ps[4:] undecayed at 3 * lr.

Rounding budget of the float64 comparison (u = 2^-24 = 6e-8, five steps).  Per step and element the kernel rounds:
d = g + wd * p (one fma), buf * momentum, + (1 - dampening) * d (one fma), d + momentum * buf (Nesterov, one fma) and
p - lr * d (one fma, or a product and a difference): at most 4u relative on d and u / 2 ulp on p.  The scalars lr,
momentum, 1 - dampening and weight_decay are fp32 kernel arguments: u relative each.  So after five steps
  |p - p64| <= 5 * (u |p| + lr |d| * ~8u) ~= 3e-7 |p| + 2.4e-6 lr |d|,
against 2e-6 |p| + 1e-7: the first term is 0.15 of rtol; the second is below atol while lr |d| < 0.04, which these
learning rates (<= 3e-2, |d| of a few units at most, on the tensors whose gradients are not scaled down) keep; at
lr = 0.5 torch's own fp32 SGD leaves the bound, which is why no such rate is here.  The buffers see 3 roundings a
step on a sum of same-sized terms, 5 steps: <= 15u ~= 9e-7 of max |buf|, against rtol 1e-6 plus 1e-6 max |buf|.

The weight_decay == 0 property is checked in the form the kernel makes checkable: L2 is bypassed by a select on the
kernel argument around d = g + wd * p, so with weight_decay == 0 nothing computed depends on p but p itself -- the
momentum buffers of two parameter sets that differ in every value, infinities included, must be equal bit for bit
(0 * inf would be NaN).

Measured on the MI355X: the worst parameter error is 0.13-0.16 of the bound in every configuration, the worst buffer
error 0.10-0.12.
"""
import copy

import pytest
import torch

from seg_amd import SGD
from seg_amd._lib import call
from seg_amd.optim import _CHUNK, _grad_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 1344, 3, 3), (10,), (3,), (4097,), (96, 16, 1, 1), (1,), (4096,), (4095,), (1000, 1280)]
CONFIGS = {"nesterov_wd": dict(momentum=0.9, nesterov=True, weight_decay=5e-4),
           "dampening": dict(momentum=0.9, dampening=0.5, weight_decay=0.0),
           "plain_wd": dict(momentum=0.0, weight_decay=1e-2),
           "momentum": dict(momentum=0.9, weight_decay=0.0)}
STEPS = 5


def _host_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in SHAPES]


def _host_grads(g):
    """One step's fp32 gradients on the host: scaled per tensor, zeros in tensor 1, none for the last tensor."""
    out = []
    for i, s in enumerate(SHAPES[:-1]):
        gr = torch.randn(s, generator=g) * 10.0 ** (-(i % 4) * 3)
        if i == 1:
            gr[::2] = 0
        out.append(gr)
    return out + [None]


@pytest.fixture(scope="module")
def inputs():
    """The starting parameters and five steps of gradients, on the host and on the device; never written."""
    g = torch.Generator().manual_seed(1)
    grads = [_host_grads(g) for _ in range(STEPS)]
    dev = [[None if t is None else t.to(DEV) for t in step] for step in grads]
    return _host_params(), grads, dev


def _params(inputs):
    return [torch.nn.Parameter(p.to(DEV)) for p in inputs[0]]


def _set(ps, step_grads):
    for p, g in zip(ps, step_grads):
        p.grad = None if g is None else g.clone()


def _groups(ps, lr, wd):
    return [{"params": ps[:4], "weight_decay": wd}, {"params": ps[4:], "weight_decay": 0.0, "lr": 3 * lr}]


def _make(cls, ps, lr, cfg, **kw):
    cfg = dict(cfg)
    return cls(_groups(ps, lr, cfg.pop("weight_decay")), lr=lr, **cfg, **kw)


def _run(inputs, lr, cfg, steps=STEPS, **step_kw):
    ps = _params(inputs)
    opt = _make(SGD, ps, lr, cfg)
    for s in range(steps):
        _set(ps, inputs[2][s])
        opt.step(**step_kw)
    torch.cuda.synchronize()
    return ps, opt


def _state_equal(oa, pa, ob, pb):
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
        assert sa.keys() == sb.keys()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k


@pytest.fixture(scope="module")
def reference(inputs):
    """(cfg name, lr) -> torch.optim.SGD in float64 on the CPU, five steps under LambdaLR(1 / (1 + e)), fed the same
    fp32 gradients cast to double: (parameters, buffers or None, the groups' final lr).  Computed once per key."""
    done = {}

    def get(name, lr):
        if (name, lr) not in done:
            ps = [torch.nn.Parameter(p.double()) for p in inputs[0]]
            opt = _make(torch.optim.SGD, ps, lr, CONFIGS[name])
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1 + e))
            for s in range(STEPS):
                for p, g in zip(ps, inputs[1][s]):
                    p.grad = None if g is None else g.double()
                opt.step()
                sched.step()
            done[(name, lr)] = ([p.detach() for p in ps], [opt.state[p].get("momentum_buffer") for p in ps],
                                [g["lr"] for g in opt.param_groups])
        return done[(name, lr)]
    return get


@pytest.mark.parametrize("lr", [1.5e-4, 1e-2])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_matches_float64(inputs, reference, name, lr):
    cfg = CONFIGS[name]
    ref_p, ref_b, ref_lr = reference(name, lr)
    ps = _params(inputs)
    opt = _make(SGD, ps, lr, cfg)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1 + e))
    for s in range(STEPS):
        _set(ps, inputs[2][s])
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    assert [g["lr"] for g in opt.param_groups] == ref_lr
    worst_p = worst_b = 0.0
    for p, r in zip(ps, ref_p):
        err = (p.detach().cpu().double() - r).abs()
        worst_p = max(worst_p, float((err / (1e-7 + 2e-6 * r.abs())).max()))
    for p, r in zip(ps[:-1], ref_b[:-1]):
        if r is not None:
            b = opt.state[p]["momentum_buffer"]
            err = (b.cpu().double() - r).abs()
            worst_b = max(worst_b, float((err / (1e-6 * float(r.abs().max()) + 1e-6 * r.abs())).max()))
    print(f"{name} lr {lr}: worst parameter error {worst_p:.3f} of the bound, worst buffer error {worst_b:.3f}")
    for i, (p, r) in enumerate(zip(ps, ref_p)):
        torch.testing.assert_close(p.detach().cpu().double(), r, rtol=2e-6, atol=1e-7, msg=lambda m: f"tensor {i}: {m}")
    assert not torch.equal(ps[0].detach().cpu(), inputs[0][0])
    assert torch.equal(ps[-1].detach().cpu(), inputs[0][-1])  # no gradient: not in the table
    assert ps[-1] not in opt.state  # (opt.state is a defaultdict: looked at without creating entries)
    for i, (p, r) in enumerate(zip(ps[:-1], ref_b[:-1])):
        if cfg["momentum"] == 0:
            assert r is None and p not in opt.state  # no buffer is ever allocated
            continue
        assert list(opt.state[p]) == ["momentum_buffer"]
        b = opt.state[p]["momentum_buffer"]
        assert b.dtype == torch.float32 and b.shape == p.shape
        torch.testing.assert_close(b.cpu().double(), r, rtol=1e-6, atol=1e-6 * float(r.abs().max()),
                                   msg=lambda m: f"buffer {i}: {m}")
    assert len(opt.state_dict()["state"]) == (0 if cfg["momentum"] == 0 else len(SHAPES) - 1)


def test_first_step_with_dampening_seeds_the_buffer_with_the_gradient(inputs):
    """torch's first step clones d into the buffer, without dampening: a zero-initialised recurrence would give
    (1 - dampening) * g.  Bit patterns, so that a gradient of -0.0 stays -0.0."""
    ps = _params(inputs)
    opt = _make(SGD, ps, 1e-2, CONFIGS["dampening"])
    grads = [None if g is None else g.clone() for g in inputs[2][0]]
    grads[1][::4] = -0.0
    _set(ps, grads)
    opt.step()
    torch.cuda.synchronize()
    for p, g in zip(ps[:-1], grads):
        b = opt.state[p]["momentum_buffer"]
        assert torch.equal(b, g)
        assert torch.equal(b.view(torch.int32), g.view(torch.int32))
        assert torch.equal(p.grad, g)  # .grad is not written
    assert bool((opt.state[ps[1]]["momentum_buffer"].view(torch.int32)[::4] == -2 ** 31).all())
    # the second step is the recurrence, on that seed: buf = g0 * 0.9 + 0.5 * g1
    _set(ps, inputs[2][1])
    opt.step()
    b, g0, g1 = opt.state[ps[3]]["momentum_buffer"].double(), grads[3].double(), inputs[2][1][3].double()
    torch.testing.assert_close(b, g0 * 0.9 + 0.5 * g1, rtol=1e-6, atol=1e-6 * float(b.abs().max()))


def test_fused_grad_scale_is_scaling_in_place_bitwise(inputs):
    cfg, lr = CONFIGS["nesterov_wd"], 1e-2
    pa, pb = _params(inputs), _params(inputs)
    oa, ob = _make(SGD, pa, lr, cfg), _make(SGD, pb, lr, cfg)
    scale = torch.tensor([0.37], device=DEV)
    for s in range(2):
        _set(pa, inputs[2][s])
        _set(pb, inputs[2][s])
        oa.step(grad_scale=scale)
        assert all(torch.equal(p.grad, g) for p, g in zip(pa[:-1], inputs[2][s]))  # .grad is not written
        live = [p for p in pb if p.grad is not None]
        table, cm = _grad_table(live)
        call("seg_grad_scale", table.data_ptr(), cm.data_ptr(), cm.shape[0], _CHUNK, scale.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
        assert all(torch.equal(p.grad, g * scale) for p, g in zip(live, inputs[2][s]))
        ob.step()
    _state_equal(oa, pa, ob, pb)
    pc, _ = _run(inputs, lr, cfg, steps=2)
    assert not torch.equal(pa[0], pc[0])  # and the scale did something


def test_zero_weight_decay_bypasses_l2_bitwise(inputs):
    """weight_decay == 0 (module docstring): the buffers do not depend on the parameters, whatever they hold."""
    cfg, lr = CONFIGS["dampening"], 1e-2
    pa, oa = _run(inputs, lr, cfg, steps=2)
    pb = [torch.nn.Parameter((p.detach() * -3.0e30 + 1.0).contiguous()) for p in _params(inputs)]
    with torch.no_grad():
        pb[3][4096] = float("inf")   # the one element of the tensor's second chunk
        pb[2][1] = float("-inf")
    ob = _make(SGD, pb, lr, cfg)  # both groups of this configuration have weight_decay 0.0
    assert [g["weight_decay"] for g in ob.param_groups] == [0.0, 0.0]
    for s in range(2):
        _set(pb, inputs[2][s])
        ob.step()
    torch.cuda.synchronize()
    for a, b in zip(pa[:-1], pb[:-1]):
        ba, bb = oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"]
        assert bool(torch.isfinite(bb).all())
        assert torch.equal(ba.view(torch.int32), bb.view(torch.int32))
    # with a weight decay the same parameters do reach the buffer
    oc = SGD([pb[3]], lr=lr, momentum=0.9, weight_decay=5e-4)
    oc.step()
    assert not bool(torch.isfinite(oc.state[pb[3]]["momentum_buffer"]).all())


@pytest.mark.parametrize("name", ["nesterov_wd", "plain_wd"])
def test_two_runs_agree_bitwise(inputs, name):
    (pa, oa), (pb, ob) = _run(inputs, 1e-2, CONFIGS[name], steps=3), _run(inputs, 1e-2, CONFIGS[name], steps=3)
    _state_equal(oa, pa, ob, pb)


def test_skip_flag(inputs):
    cfg, lr = CONFIGS["nesterov_wd"], 1e-2
    pa, pb = _params(inputs), _params(inputs)
    oa, ob = _make(SGD, pa, lr, cfg), _make(SGD, pb, lr, cfg)
    one, zero, half = (torch.tensor([v], device=DEV) for v in (1.0, 0.0, 0.5))
    for ps, o in ((pa, oa), (pb, ob)):
        _set(ps, inputs[2][0])
        o.step(grad_scale=half)
    _set(pa, inputs[2][1])
    _set(pb, inputs[2][1])
    keep = [(p.detach().clone(), oa.state[p]["momentum_buffer"].clone()) for p in pa[:-1]]
    oa.step(skip_if_nonzero=one, grad_scale=half)
    oa.undo_step_count()  # nothing was created by that step: nothing goes
    for p, (p0, b0) in zip(pa[:-1], keep):
        assert torch.equal(p, p0) and list(oa.state[p]) == ["momentum_buffer"]
        assert torch.equal(oa.state[p]["momentum_buffer"], b0)
    oa.step(skip_if_nonzero=zero, grad_scale=half)
    ob.step(grad_scale=half)
    _state_equal(oa, pa, ob, pb)


@pytest.mark.parametrize("name", ["nesterov_wd", "dampening"])
def test_skipped_first_step_leaves_no_state(inputs, name):
    cfg, lr = CONFIGS[name], 1e-2
    pa = _params(inputs)
    oa = _make(SGD, pa, lr, cfg)
    before = oa.state_dict()
    assert before["state"] == {}
    one = torch.tensor([3.0], device=DEV)
    _set(pa, inputs[2][0])
    oa.step(skip_if_nonzero=one)
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach().cpu(), p0) for p, p0 in zip(pa, inputs[0]))
    assert all(not bool(oa.state[p]["momentum_buffer"].any()) for p in pa[:-1])  # created at queue time, untouched
    oa.undo_step_count()
    after = oa.state_dict()
    assert after["state"] == {} and after["param_groups"] == before["param_groups"]
    oa.step()  # the real first step: torch's, buf = d
    pb, ob = _run(inputs, lr, cfg, steps=1)
    _state_equal(oa, pa, ob, pb)
    assert torch.equal(oa.state[pa[5]]["momentum_buffer"], inputs[2][0][5])  # tensor 5 is undecayed: buf = g


def test_checkpoints_move_both_ways(inputs):
    cfg, lr = CONFIGS["nesterov_wd"], 1e-2
    full_p, full_o = _run(inputs, lr, cfg)                      # ours, five steps
    pt = _params(inputs)
    ot = _make(torch.optim.SGD, pt, lr, cfg, foreach=True)      # torch, two steps
    for s in range(2):
        _set(pt, inputs[2][s])
        ot.step()
    ours_p = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    ours = _make(SGD, ours_p, lr, cfg)
    ours.load_state_dict(copy.deepcopy(ot.state_dict()))  # load_state_dict keeps same-dtype tensors as they are
    assert ours.state_dict()["param_groups"][0].keys() == ot.state_dict()["param_groups"][0].keys()
    assert ours.state_dict()["state"].keys() == ot.state_dict()["state"].keys()
    loaded = [ours.state[p]["momentum_buffer"].clone() for p in ours_p[:-1]]
    for s in range(2, STEPS):
        _set(ours_p, inputs[2][s])
        ours.step()
        assert ours._last_seeded == []  # the loaded buffers continue the recurrence: nothing is seeded again
    torch.cuda.synchronize()
    assert not torch.equal(ours.state[ours_p[0]]["momentum_buffer"], loaded[0])
    for i, (a, b) in enumerate(zip(ours_p, full_p)):
        torch.testing.assert_close(a, b, rtol=2e-6, atol=1e-7, msg=lambda m: f"tensor {i}: {m}")
    for a, b in zip(ours_p[:-1], full_p[:-1]):
        ba, bb = ours.state[a]["momentum_buffer"], full_o.state[b]["momentum_buffer"]
        torch.testing.assert_close(ba, bb, rtol=1e-6, atol=1e-6 * float(bb.abs().max()))
    # and back: torch continues from our state
    back_p = [torch.nn.Parameter(p.detach().clone()) for p in full_p]
    back = _make(torch.optim.SGD, back_p, lr, cfg, foreach=True)
    back.load_state_dict(copy.deepcopy(full_o.state_dict()))
    again_p = [torch.nn.Parameter(p.detach().clone()) for p in full_p]
    again = _make(SGD, again_p, lr, cfg)
    again.load_state_dict(copy.deepcopy(full_o.state_dict()))
    for ps, o in ((back_p, back), (again_p, again)):
        _set(ps, inputs[2][0])
        o.step()
    for i, (a, b) in enumerate(zip(back_p, again_p)):
        torch.testing.assert_close(b, a, rtol=2e-6, atol=1e-7, msg=lambda m: f"tensor {i}: {m}")
    assert not back.state.get(back_p[-1]) and again_p[-1] not in again.state


# ---------------------------------------------------------------- refusals on CUDA tensors
#
# The kernel indexes p, p.grad and the buffer flatly through raw pointers, so everything that is not a dense
# contiguous fp32 tensor has to stop on the host.  On CUDA tensors each clause of the check is the one that decides
# (a CPU tensor always fails on the device clause first: tests/test_optim_sgd.py).  A refused step launches nothing
# and creates nothing: the good parameter in front of the bad one, in a group of its own, stays bit for bit where it
# was and the optimizer's state stays empty.

def _good():
    g = torch.Generator().manual_seed(5)
    p = torch.nn.Parameter(torch.randn(8, 4, generator=g).to(DEV))
    p.grad = torch.randn(8, 4, generator=g).to(DEV)
    return p


def _noncontiguous_parameter():
    p = torch.nn.Parameter(torch.randn(4, 8, device=DEV).t())
    p.grad = torch.randn(8, 4, device=DEV)
    return p


def _noncontiguous_gradient():
    p = torch.nn.Parameter(torch.randn(8, 4, device=DEV))
    p.grad = torch.randn(4, 8, device=DEV).t()
    return p


def _other_dtype(dtype):
    def make():
        p = torch.nn.Parameter(torch.randn(8, 4, device=DEV).to(dtype))
        p.grad = torch.randn(8, 4, device=DEV).to(dtype)
        return p
    return make


def _sparse_gradient():
    p = torch.nn.Parameter(torch.randn(8, 4, device=DEV))
    i = torch.tensor([[0, 3], [1, 2]], device=DEV)
    p.grad = torch.sparse_coo_tensor(i, torch.ones(2, device=DEV), (8, 4))
    return p


BAD_TENSORS = {"noncontiguous_parameter": _noncontiguous_parameter, "noncontiguous_gradient": _noncontiguous_gradient,
               "fp16": _other_dtype(torch.float16), "fp64": _other_dtype(torch.float64),
               "sparse_gradient": _sparse_gradient}


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("case", list(BAD_TENSORS))
def test_refuses_cuda_tensors_it_cannot_index(case, momentum):
    good, bad = _good(), BAD_TENSORS[case]()
    assert bad.is_cuda and bad.grad.is_cuda
    if case == "noncontiguous_parameter":
        assert not bad.is_contiguous() and bad.grad.is_contiguous() and bad.dtype == torch.float32
    if case == "noncontiguous_gradient":
        assert bad.is_contiguous() and not bad.grad.is_contiguous()
    if case == "sparse_gradient":
        assert bad.grad.is_sparse and bad.grad.dtype == torch.float32 and bad.is_contiguous()
    start, bad_start = good.detach().clone(), bad.detach().clone()
    opt = SGD([{"params": [good]}, {"params": [bad]}], lr=1e-2, momentum=momentum, weight_decay=5e-4)
    with pytest.raises(NotImplementedError):
        opt.step()
    torch.cuda.synchronize()
    assert len(opt.state) == 0 and opt.state_dict()["state"] == {}
    assert torch.equal(good, start) and torch.equal(bad, bad_start)  # not even the good group was launched
    opt.undo_step_count()  # nothing to take back
    # the same optimizer steps once the offending tensor has no gradient
    bad.grad = None
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(good, start) and torch.equal(bad, bad_start)
    assert len(opt.state) == (1 if momentum else 0)


def _transposed(p):
    return torch.zeros(p.shape[::-1], device=DEV).t()


@pytest.mark.parametrize("case", ["fp16", "fp64", "noncontiguous", "shape", "cpu", "loaded_noncontiguous"])
def test_refuses_a_momentum_buffer_it_cannot_index(case):
    good, other = _good(), _good()
    start, other_start = good.detach().clone(), other.detach().clone()
    opt = SGD([{"params": [good]}, {"params": [other]}], lr=1e-2, momentum=0.9)
    if case == "loaded_noncontiguous":  # load_state_dict casts dtype and device to the parameter's; the layout stays
        sd = opt.state_dict()
        sd["state"] = {1: {"momentum_buffer": _transposed(other)}}
        opt.load_state_dict(sd)
        assert not opt.state[other]["momentum_buffer"].is_contiguous()
    else:
        buf = {"fp16": lambda: torch.zeros_like(other, dtype=torch.float16),
               "fp64": lambda: torch.zeros_like(other, dtype=torch.float64),
               "noncontiguous": lambda: _transposed(other),
               "shape": lambda: torch.zeros(other.numel() - 1, device=DEV),
               "cpu": lambda: torch.zeros(other.shape)}[case]()
        opt.state[other]["momentum_buffer"] = buf
    kept = opt.state[other]["momentum_buffer"]
    with pytest.raises(NotImplementedError):
        opt.step()
    torch.cuda.synchronize()
    assert good not in opt.state  # checked before the first buffer is created and the first launch queued
    assert opt.state[other]["momentum_buffer"] is kept and not bool(kept.any())
    assert torch.equal(good, start) and torch.equal(other, other_start)
    # with momentum 0 the buffer is not part of the step: never read, so not refused either
    plain = SGD([{"params": [good]}, {"params": [other]}], lr=1e-2)
    plain.state[other]["momentum_buffer"] = kept
    plain.step()
    torch.cuda.synchronize()
    assert not torch.equal(other, other_start) and not bool(kept.any())


def test_momentum_that_underflows_in_fp32_is_no_momentum(inputs):
    """The entry point picks the kernel on the fp32 value of momentum; the host decides on the same value, so no
    buffer is created that no kernel would write."""
    cfg = dict(CONFIGS["plain_wd"])
    pa, oa = _run(inputs, 1e-2, cfg, steps=2)
    pb, ob = _run(inputs, 1e-2, dict(cfg, momentum=1e-50), steps=2)
    assert ob.param_groups[0]["momentum"] == 1e-50 and len(ob.state) == 0 and ob.state_dict()["state"] == {}
    _state_equal(oa, pa, ob, pb)
