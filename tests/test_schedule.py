"""CPU: seg_amd.PolyLR -- the poly decay against torch's PolynomialLR, the warm-up and min_lr against the formula
of seg_amd/schedule.py written out here, the argument checks, and resume from state_dict()."""
import pytest
import torch

from seg_amd import PolyLR


def _opt(lrs=(1e-2,)):
    groups = [{"params": [torch.nn.Parameter(torch.zeros(2))], "lr": lr} for lr in lrs]
    return torch.optim.SGD(groups, lr=lrs[0], momentum=0.9)


def _run(opt, sched, n):
    """The learning rates of every group at iterations 0 .. n-1 (optimizer.step() then scheduler.step())."""
    out = []
    for _ in range(n):
        out.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("power", [0.9, 1.0, 2.0])
def test_plain_poly_is_torchs_polynomial_lr(power):
    T = 7
    oa, ob = _opt(), _opt()
    ours = _run(oa, PolyLR(oa, total_iters=T, power=power), T + 3)  # past T: the clamp
    ref = _run(ob, torch.optim.lr_scheduler.PolynomialLR(ob, total_iters=T, power=power), T + 3)
    assert len(ours) == T + 3
    for t, (a, b) in enumerate(zip(ours, ref)):
        assert a[0] == pytest.approx(b[0], rel=1e-12, abs=0.0), t
    assert ours[0][0] == 1e-2 and ours[T][0] == 0.0 and ours[T + 2][0] == 0.0
    assert all(x[0] > y[0] for x, y in zip(ours[:T], ours[1:T + 1]))  # strictly decreasing down to the clamp


def test_warmup_and_min_lr_follow_the_formula():
    T, W, ratio, power, min_lr = 20, 5, 0.25, 0.9, 1e-4
    bases = (1e-2, 3e-2)
    opt = _opt(bases)
    got = _run(opt, PolyLR(opt, total_iters=T, power=power, min_lr=min_lr, warmup_iters=W, warmup_ratio=ratio), T + 2)
    for t, lrs in enumerate(got):
        for base, lr in zip(bases, lrs):
            poly = min_lr + (base - min_lr) * (1 - min(t, T) / T) ** power
            want = poly * (ratio + (1 - ratio) * t / W) if t < W else poly
            assert lr == pytest.approx(want, rel=1e-12, abs=0.0), (t, base)
    assert got[0] == [b * ratio for b in bases]  # t = 0: poly(0) = base exactly
    assert got[T] == got[T + 1] == [min_lr, min_lr]
    assert got[3][1] != pytest.approx(3 * got[3][0])  # min_lr is not scaled with the base rate


def test_t0_and_continuity_at_the_end_of_warmup():
    base, T, W = 1e-2, 100, 10
    opt = _opt((base,))
    sched = PolyLR(opt, total_iters=T, warmup_iters=W)  # warmup_ratio 0.1
    assert opt.param_groups[0]["lr"] == base * 0.1
    lrs = [lr[0] for lr in _run(opt, sched, W + 2)]
    poly = lambda t: base * (1 - t / T) ** 0.9  # noqa: E731
    assert lrs[W] == pytest.approx(poly(W), rel=1e-12)  # the warm-up factor has reached 1: no jump
    # the last warm-up value approaches poly(W) from below by one warm-up increment, not more
    assert lrs[W - 1] == pytest.approx(poly(W - 1) * (0.1 + 0.9 * (W - 1) / W), rel=1e-12)
    assert lrs[W - 1] < lrs[W] and lrs[W + 1] < lrs[W]
    assert lrs[W] - lrs[W - 1] < 1.01 * (lrs[1] - lrs[0])
    opt = _opt((base,))
    PolyLR(opt, total_iters=T, warmup_iters=W, warmup_ratio=1.0)  # ratio 1: no warm-up at all
    assert opt.param_groups[0]["lr"] == base


def test_argument_errors():
    for kw in ({"total_iters": 0}, {"total_iters": 5, "power": 0.0}, {"total_iters": 5, "power": -1.0},
               {"total_iters": 5, "warmup_iters": 5}, {"total_iters": 5, "warmup_iters": -1},
               {"total_iters": 5, "warmup_ratio": 0.0}, {"total_iters": 5, "warmup_ratio": 1.5},
               {"total_iters": 5, "min_lr": -1e-6}, {"total_iters": 5, "min_lr": 1e-2},
               {"total_iters": 5, "min_lr": 2e-2}):
        with pytest.raises(ValueError):
            PolyLR(_opt((3e-2, 1e-2)), **kw)  # min_lr is checked against every group: the second one's 1e-2
    PolyLR(_opt((3e-2, 1e-2)), total_iters=1)
    PolyLR(_opt((3e-2, 1e-2)), total_iters=5, warmup_iters=4, warmup_ratio=1.0, min_lr=9e-3)


def test_resume_from_state_dict():
    kw = dict(total_iters=12, power=0.9, min_lr=1e-4, warmup_iters=3, warmup_ratio=0.2)
    opt = _opt((1e-2, 3e-2))
    full = _run(opt, PolyLR(opt, **kw), 14)
    o1 = _opt((1e-2, 3e-2))
    s1 = PolyLR(o1, **kw)
    head = _run(o1, s1, 5)
    o2 = _opt((1e-2, 3e-2))
    s2 = PolyLR(o2, **kw)  # a fresh pair, then both states: torch's resume order
    o2.load_state_dict(o1.state_dict())
    s2.load_state_dict(s1.state_dict())
    assert set(s1.state_dict()) >= {"last_epoch", "total_iters", "power", "min_lr", "warmup_iters", "warmup_ratio"}
    assert s2.last_epoch == 5
    tail = _run(o2, s2, 9)
    assert head + tail == full
    assert s2.get_last_lr() == [g["lr"] for g in o2.param_groups]
