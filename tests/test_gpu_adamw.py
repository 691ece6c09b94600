"""GPU: seg_amd.AdamW (seg_adamw_step), grad_norm (seg_grad_sumsq) and clip_grad_norm_ (seg_grad_scale) of
csrc/adam.hip against torch.optim.AdamW(foreach=True), a float64 norm and torch.nn.utils.clip_grad_norm_.

Shapes: tests/test_gpu_adam.py's plus 4096 and 4095 elements (the chunk edge) and a last (1000, 1280) tensor
without a gradient.  The tensors with a gradient make 764 chunks; the norm is also taken with the last tensor's
gradient present (1077 chunks), so the one-block finalize walks its partials more than once per thread.

Tolerances.  The step: tests/test_gpu_adam.py's (same operations in the same order).  The norm: each element
enters one fma of a serial chain of <= 16 (4096 / 256), then 6 butterfly levels in the wave and 2 over the four
waves, all fp32 on non-negative terms: relative error of a partial <= 24 * 2^-24 = 1.4e-6; the partials are added
in double; the square root halves the relative error and rounds once: < 8e-7 on the norm, against rtol 1e-5.
The clipped gradients: the coefficient's 1e-5 plus one rounding, rtol 2e-5.
"""
import pytest
import torch

from seg_amd import Adam, AdamW, clip_grad_norm_, grad_norm
from seg_amd._lib import call
from seg_amd.optim import _CHUNK, _grad_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 1344, 3, 3), (10,), (3,), (4097,), (96, 16, 1, 1), (1,), (4096,), (4095,), (1000, 1280)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in SHAPES]


def _set_grads(lists, g, last=False):
    """The existing test's gradients (scaled per tensor, zeros in tensor 1) on every list of parameters alike."""
    for i, ps in enumerate(zip(*lists)):
        if i == len(SHAPES) - 1 and not last:
            for p in ps:
                p.grad = None
            continue
        gr = (torch.randn(ps[0].shape, generator=g) * 10.0 ** (-(i % 4) * 3)).to(DEV)
        if i == 1:
            gr[::2] = 0  # zero gradients: v == 0 -> denominator eps
        for p in ps:
            p.grad = gr.clone()


def _groups(ps, lr):
    return [{"params": ps[:4], "weight_decay": 1e-2}, {"params": ps[4:], "weight_decay": 0.0, "lr": 3 * lr}]


def _state_equal(oa, pa, ob, pb):
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        sa, sb = oa.state[a], ob.state[b]
        assert sa.keys() == sb.keys()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k


@pytest.fixture(scope="module")
def grads():
    """Parameters with the test gradients on every tensor but the last, one set with it too, and the float64 norms."""
    ps, full = _params(0), _params(0)
    _set_grads([ps], torch.Generator().manual_seed(1))
    _set_grads([full], torch.Generator().manual_seed(1), last=True)
    ref = lambda qs: float(torch.sqrt(sum((q.grad.double() ** 2).sum() for q in qs if q.grad is not None)))  # noqa: E731
    return ps, ref(ps), full, ref(full)


@pytest.mark.parametrize("lr", [1.5e-4, 1e-2])
def test_adamw_matches_torch(lr):
    ref, ours = _params(0), _params(0)
    o_ref = torch.optim.AdamW(_groups(ref, lr), lr=lr, foreach=True)
    o_ours = AdamW(_groups(ours, lr), lr=lr)
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, lambda e: 1.0 / (1 + e)) for o in (o_ref, o_ours)]
    g = torch.Generator().manual_seed(1)
    for step in range(5):
        _set_grads([ref, ours], g)
        o_ref.step()
        o_ours.step()
        for s in scheds:
            s.step()
    torch.cuda.synchronize()
    assert [gr["lr"] for gr in o_ours.param_groups] == [gr["lr"] for gr in o_ref.param_groups]
    for a, b in zip(ref, ours):
        torch.testing.assert_close(b, a, rtol=2e-6, atol=1e-7)
    assert not torch.equal(ours[0], _params(0)[0])
    for a, b in zip(ref[:-1], ours[:-1]):
        sa, sb = o_ref.state[a], o_ours.state[b]
        assert float(sa["step"]) == float(sb["step"]) == 5.0
        for k in ("exp_avg", "exp_avg_sq"):
            torch.testing.assert_close(sb[k], sa[k], rtol=1e-6, atol=1e-6 * float(sa[k].abs().max()))
    assert len(o_ours.state[ours[-1]]) == 0
    # checkpoint compatibility, both directions
    o2 = AdamW(_groups(_params(0), lr), lr=lr)
    o2.load_state_dict(o_ref.state_dict())
    o3 = torch.optim.AdamW(_groups(_params(0), lr), lr=lr)
    o3.load_state_dict(o_ours.state_dict())
    assert o_ours.state_dict()["param_groups"][0].keys() == o_ref.state_dict()["param_groups"][0].keys()


def test_weight_decay_is_applied():
    """Decay alone moves a parameter whose gradient is zero: p * (1 - lr * wd), then no Adam update."""
    p = torch.nn.Parameter(torch.full((5000,), 2.0, device=DEV))
    p.grad = torch.zeros_like(p)
    AdamW([p], lr=0.1, weight_decay=0.5).step()
    assert torch.equal(p.detach(), torch.full_like(p, 2.0) * 0.95)


def test_zero_weight_decay_is_adam_bitwise():
    pa, pw = _params(0), _params(0)
    oa, ow = Adam(pa, lr=1e-2), AdamW(pw, lr=1e-2, weight_decay=0.0)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        _set_grads([pa, pw], g)
        oa.step()
        ow.step()
    _state_equal(oa, pa[:-1], ow, pw[:-1])


@pytest.mark.parametrize("c", [1.0, 0.37])
@pytest.mark.parametrize("cls", [Adam, AdamW])
def test_fused_grad_scale_is_scaling_in_place_bitwise(cls, c):
    pa, pb = _params(0), _params(0)
    oa, ob = cls(pa, lr=1e-2), cls(pb, lr=1e-2)
    scale = torch.tensor([c], device=DEV)
    g = torch.Generator().manual_seed(1)
    for _ in range(2):
        _set_grads([pa, pb], g)
        before = [p.grad.clone() for p in pa[:-1]]
        oa.step(grad_scale=scale)
        assert all(torch.equal(p.grad, b) for p, b in zip(pa, before))  # .grad is not written
        live = [p for p in pb if p.grad is not None]
        table, cm = _grad_table(live)
        call("seg_grad_scale", table.data_ptr(), cm.data_ptr(), cm.shape[0], _CHUNK, scale.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
        assert all(torch.equal(p.grad, b * scale) for p, b in zip(live, before))
        ob.step()
    _state_equal(oa, pa[:-1], ob, pb[:-1])


def test_grad_norm(grads):
    ps, ref, full, ref_full = grads
    for qs, want in ((ps, ref), (full, ref_full)):
        a, b = grad_norm(qs, 1.0), grad_norm(qs, 1.0)
        assert a.shape == (3,) and a.dtype == torch.float32 and a.is_cuda
        assert torch.equal(a, b)  # fixed summation order: bitwise the same run to run
        print(f"norm {float(a[0]):.9g} float64 {want:.9g} rel {abs(float(a[0]) - want) / want:.2e}")
        assert abs(float(a[0]) - want) <= 1e-5 * want
        tn = torch.nn.utils.get_total_norm([q.grad for q in qs if q.grad is not None])
        torch.testing.assert_close(a[0], tn, rtol=1e-5, atol=0)
        assert float(a[2]) == 0.0
        assert float(a[1]) == float(torch.tensor(1.0) / (a[0].cpu() + 1e-6))
    assert ref_full > ref
    assert grad_norm(ps).tolist()[1:] == [1.0, 0.0]          # no max_norm: coefficient 1
    assert float(grad_norm(ps, float("inf"))[1]) == 1.0
    assert torch.equal(grad_norm(ps[:3])[0], grad_norm(ps[:3] + [ps[-1]])[0])  # grad None is ignored
    assert grad_norm([ps[-1]]).tolist() == [0.0, 1.0, 0.0] and grad_norm([ps[-1]]).is_cuda


def _clones(ps):
    out = []
    for p in ps:
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = None if p.grad is None else p.grad.clone()
        out.append(q)
    return out


def test_clip_above(grads):
    ps, ref = grads[0], grads[1]
    a, b = _clones(ps), _clones(ps)
    max_norm = ref / 2
    n = clip_grad_norm_(a, max_norm)
    nt = torch.nn.utils.clip_grad_norm_(b, max_norm)
    assert n.ndim == 0 and n.is_cuda
    torch.testing.assert_close(n, nt, rtol=1e-5, atol=0)
    assert a[-1].grad is None
    for p, q, o in zip(a[:-1], b[:-1], ps):
        torch.testing.assert_close(p.grad, q.grad, rtol=2e-5, atol=0)
        assert not torch.equal(p.grad, o.grad) or not bool(o.grad.any())
    assert abs(float(grad_norm(a)[0]) - max_norm) <= 3e-5 * max_norm


def test_clip_below_leaves_gradients_alone(grads):
    ps, ref = grads[0], grads[1]
    a = _clones(ps)
    assert float(grad_norm(a, 2 * ref)[1]) == 1.0
    n = clip_grad_norm_(a, 2 * ref)
    assert abs(float(n) - ref) <= 1e-5 * ref
    assert all(torch.equal(p.grad, o.grad) for p, o in zip(a[:-1], ps))


def test_clip_zero_gradients():
    a = _params(0)[:6]
    for p in a:
        p.grad = torch.zeros_like(p)
    out = grad_norm(a, 1.0)
    assert out.tolist() == [0.0, 1.0, 0.0]
    assert float(clip_grad_norm_(a, 1.0)) == 0.0
    assert all(not bool(p.grad.any()) for p in a)  # all zero still: nothing became NaN


def test_clip_nonfinite(grads):
    ps = grads[0]
    a, b = _clones(ps), _clones(ps)
    for qs in (a, b):
        qs[3].grad[4096] = float("inf")  # the one element of the tensor's second chunk
    assert float(grad_norm(a, 1.0)[2]) == 1.0
    with pytest.raises(RuntimeError):
        clip_grad_norm_(a, 1.0, error_if_nonfinite=True)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a[:-1], b[:-1]))  # the refused clip wrote nothing
    n = clip_grad_norm_(a, 1.0)
    nt = torch.nn.utils.clip_grad_norm_(b, 1.0)
    assert torch.equal(n, nt) and float(n) == float("inf")
    for p, q in zip(a[:-1], b[:-1]):
        assert torch.allclose(p.grad, q.grad, rtol=0, atol=0, equal_nan=True)
    assert bool(torch.isnan(a[3].grad[4096]))
    a[0].grad[0, 0, 0, 0] = float("nan")
    out = grad_norm(a, 1.0)
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[1])) and float(out[2]) == 1.0


@pytest.mark.parametrize("cls", [Adam, AdamW])
def test_skip_flag(cls):
    pa, pb = _params(0), _params(0)
    oa, ob = cls(pa, lr=1e-2), cls(pb, lr=1e-2)
    g = torch.Generator().manual_seed(1)
    one, zero, half = (torch.tensor([v], device=DEV) for v in (1.0, 0.0, 0.5))
    _set_grads([pa, pb], g)
    oa.step(grad_scale=half)
    ob.step(grad_scale=half)
    _set_grads([pa, pb], g)
    keep = [(p.detach().clone(), {k: v.clone() for k, v in oa.state[p].items()}) for p in pa[:-1]]
    oa.step(skip_if_nonzero=one, grad_scale=half)
    assert all(float(oa.state[p]["step"]) == 2.0 for p in pa[:-1])
    oa.undo_step_count()
    for p, (p0, st0) in zip(pa[:-1], keep):
        assert torch.equal(p, p0)
        assert all(torch.equal(oa.state[p][k], st0[k]) for k in st0)  # moments and step == 1
    oa.step(skip_if_nonzero=zero, grad_scale=half)
    ob.step(grad_scale=half)
    _state_equal(oa, pa[:-1], ob, pb[:-1])
