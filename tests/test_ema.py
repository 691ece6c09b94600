"""CPU: seg_amd.EMA on the torch-op composition -- what it covers, the recurrence, the warm-up schedule, the
in-place exchange, the averaged state_dict, resuming, rebinding, and train_model(..., ema=).

Bound against the float64 recurrence e64 += double(w_fp32) * (p - e64): after k updates |e - e64| <= k * 2^-21 * M,
M the largest |e| or |p| the element has seen (one rounding of p - e, <= 2^-24 * 2M, at most one of the product and
one of the sum: <= 5 * 2^-24 * M per update for w <= 1; the map contracts, so the errors at most add)."""
import json
import os

import pytest
import torch
from torch import nn

import seg_amd
from seg_amd import EMA, MobileNetV2UNet, UNet, deterministic_init, synthetic_batch, train_model
from seg_amd.ema import warmup_decay


def _tiny(seed=1):
    return deterministic_init(UNet(4, 8), seed=seed)


def _perturb(model, seed):
    """Move every floating-point state entry, as a training step would."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in model.state_dict().values():
            if v.is_floating_point():
                v.add_(0.1 * torch.randn(v.shape, generator=g))


def _batches(n, seed0=3):
    return [synthetic_batch(2, 16, 16, 4, seed=seed0 + i) for i in range(n)]


def test_covers_every_float_entry_and_no_integer_one():
    model = _tiny()
    ema = EMA(model)
    sd = model.state_dict()
    floats = [k for k, v in sd.items() if v.is_floating_point()]
    ints = [k for k, v in sd.items() if not v.is_floating_point()]
    assert ints and all(k.endswith("num_batches_tracked") for k in ints)
    assert ema.names == floats and len(ema.shadows) == len(floats)
    assert any(k.endswith("running_var") for k in ema.names) and any(k.endswith("weight") for k in ema.names)
    for k, e in zip(ema.names, ema.shadows):
        assert torch.equal(e, sd[k]) and e.data_ptr() != sd[k].data_ptr(), k  # a copy of its own
    assert ema.num_updates == 0


def test_aliased_entries_share_one_shadow():
    """MobileNetV2UNet's state_dict names some tensors twice (691 keys): each tensor is averaged once."""
    model = MobileNetV2UNet(10)
    ema = EMA(model)
    sd = model.state_dict()
    floats = [k for k, v in sd.items() if v.is_floating_point()]
    unique = {id(v) for v in list(model.parameters()) + [b for b in model.buffers() if b.is_floating_point()]}
    assert ema.names == floats and len(ema.shadows) == len(unique) < len(floats)
    _perturb(model, 5)  # (an aliased tensor moves twice: only the values matter here)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with ema.applied():
        pass
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_three_updates_equal_the_float64_recurrence():
    model = _tiny()
    decay = 0.9
    ema = EMA(model, decay=decay)
    w = float(torch.tensor(1.0 - decay, dtype=torch.float32))
    e64 = {k: v.double().clone() for k, v in model.state_dict().items() if v.is_floating_point()}
    M = {k: v.abs() for k, v in e64.items()}
    k_updates = 3
    for step in range(k_updates):
        _perturb(model, 10 + step)
        ema.update()
        for k, v in model.state_dict().items():
            if k in e64:
                e64[k] += w * (v.double() - e64[k])
                M[k] = torch.maximum(M[k], torch.maximum(v.double().abs(), e64[k].abs()))
    assert ema.num_updates == k_updates
    worst = 0.0
    for k, e in zip(ema.names, ema.shadows):
        err = (e.double() - e64[k]).abs()
        bound = k_updates * 2.0 ** -21 * M[k]
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), k
        assert not torch.equal(e, model.state_dict()[k]) or e.numel() == 0, k  # it is an average, not a copy
    print(f"worst error / bound after {k_updates} updates: {worst:.3f}")


def test_warmup_schedule():
    assert warmup_decay(0.999, 0) == 1 / 10
    assert warmup_decay(0.999, 1) == 2 / 11
    assert warmup_decay(0.999, 10) == 11 / 20
    assert warmup_decay(0.999, 10 ** 4) == 0.999  # (1 + n) / (10 + n) = 0.99910...: the cap holds
    ema = EMA(_tiny(), decay=0.999, warmup=True)
    assert ema.current_decay() == 0.1
    ema.update()
    assert ema.num_updates == 1 and ema.current_decay() == 2 / 11
    ema.undo_update_count()
    assert ema.num_updates == 0 and ema.current_decay() == 0.1
    ema.undo_update_count()  # nothing more to take back
    assert ema.num_updates == 0
    assert EMA(_tiny(), decay=0.999).current_decay() == 0.999


def test_first_warmup_update_uses_a_tenth():
    model = _tiny()
    ema = EMA(model, decay=0.999, warmup=True)
    start = [e.clone() for e in ema.shadows]
    _perturb(model, 2)
    ema.update()
    sd = model.state_dict()
    for k, e, s in zip(ema.names, ema.shadows, start):
        torch.testing.assert_close(e, s + 0.9 * (sd[k] - s), rtol=1e-5, atol=1e-7)


def test_applied_swaps_in_and_restores_bit_for_bit():
    model = _tiny()
    ema = EMA(model, decay=0.5)
    _perturb(model, 4)
    ema.update()
    live = {k: v.clone() for k, v in model.state_dict().items()}
    avg = ema.averaged_state_dict()
    assert any(not torch.equal(avg[k], live[k]) for k in ema.names)
    ptrs = [v.data_ptr() for v in model.state_dict().values()]
    with ema.applied() as inside:
        assert inside is ema
        now = model.state_dict()
        for k in now:
            assert torch.equal(now[k], avg[k]), k  # integer buffers: the live ones either way
        for k, e in zip(ema.names, ema.shadows):
            assert torch.equal(e, live[k]), k
        assert all(torch.equal(v, avg[k]) for k, v in ema.averaged_state_dict().items())
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError):
            ema.update()
        assert all(torch.equal(v, avg[k]) for k, v in model.state_dict().items())  # the refusals changed nothing
    assert [v.data_ptr() for v in model.state_dict().values()] == ptrs
    for k, v in model.state_dict().items():
        assert torch.equal(v, live[k]), k
    for k, v in ema.averaged_state_dict().items():
        assert torch.equal(v, avg[k]), k
    ema.swap()  # the same exchange by hand
    assert all(torch.equal(v, avg[k]) for k, v in model.state_dict().items())
    ema.swap()
    assert all(torch.equal(v, live[k]) for k, v in model.state_dict().items())


def test_applied_restores_after_an_exception():
    model = _tiny()
    ema = EMA(model, decay=0.5)
    _perturb(model, 4)
    ema.update()
    live = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            1 / 0
    assert all(torch.equal(v, live[k]) for k, v in model.state_dict().items())
    with ema.applied():  # and it can be entered again
        pass


@pytest.mark.parametrize("arch,ctor", [("UNet", lambda: UNet(10)), ("MobileNetV2UNet", lambda: MobileNetV2UNet(10))])
def test_averaged_state_dict_has_the_reference_keys(golden_dir, arch, ctor):
    with open(os.path.join(golden_dir, "state_dict_keys.json")) as f:
        ref = json.load(f)[arch]
    model = ctor()
    ema = EMA(model, decay=0.5)
    _perturb(model, 6)
    ema.update()
    avg = ema.averaged_state_dict()
    assert [[k, list(v.shape)] for k, v in avg.items()] == ref
    sd = model.state_dict()
    assert all(v.data_ptr() != sd[k].data_ptr() or v.numel() == 0 for k, v in avg.items())  # clones
    assert all(torch.equal(v, sd[k]) for k, v in avg.items() if not v.is_floating_point())
    fresh = ctor()
    assert fresh.load_state_dict(avg, strict=True).missing_keys == []
    other = ctor()
    ema.copy_to(other)
    assert all(torch.equal(v, avg[k]) for k, v in other.state_dict().items())
    assert all(torch.equal(v, avg[k]) for k, v in fresh.state_dict().items())


def test_state_dict_round_trip():
    model = _tiny()
    ema = EMA(model, decay=0.99, warmup=True)
    for s in range(3):
        _perturb(model, 20 + s)
        ema.update()
    state = ema.state_dict()
    assert set(state) == {"decay", "warmup", "num_updates", "shadow"}
    assert (state["decay"], state["warmup"], state["num_updates"]) == (0.99, True, 3)
    assert list(state["shadow"]) == ema.names
    path_free = {k: v.clone() for k, v in state["shadow"].items()}
    other = EMA(_tiny(seed=2), decay=0.5)
    other.load_state_dict(state)
    assert (other.decay, other.warmup, other.num_updates) == (0.99, True, 3)
    for k, e in zip(other.names, other.shadows):
        assert torch.equal(e, path_free[k]), k
    assert other.current_decay() == ema.current_decay()
    bad = dict(state, shadow={k: v for k, v in list(state["shadow"].items())[1:]})
    with pytest.raises(KeyError):
        other.load_state_dict(bad)


@pytest.mark.parametrize("decay", [1.5, -0.1, float("nan")])
def test_decay_outside_the_unit_interval_raises(decay):
    with pytest.raises(ValueError):
        EMA(_tiny(), decay=decay)


def test_decay_one_and_zero():
    model = _tiny()
    keep, follow = EMA(model, decay=1.0), EMA(model, decay=0.0)
    start = [e.clone() for e in keep.shadows]
    _perturb(model, 8)
    keep.update()
    follow.update()
    sd = model.state_dict()
    assert all(torch.equal(e, s) for e, s in zip(keep.shadows, start))
    assert all(torch.equal(e, sd[k]) for k, e in zip(follow.names, follow.shadows))


def test_rebinding_through_assign_is_followed_with_shadows_kept():
    model = _tiny()
    ema = EMA(model, decay=0.5)
    _perturb(model, 9)
    ema.update()
    shadows = [e.clone() for e in ema.shadows]
    new = {k: (v + 1 if v.is_floating_point() else v.clone()) for k, v in _tiny(seed=3).state_dict().items()}
    old_ptrs = [v.data_ptr() for v in model.state_dict().values()]
    model.load_state_dict({k: v.clone() for k, v in new.items()}, assign=True)  # the model adopts these tensors
    assert [v.data_ptr() for v in model.state_dict().values()] != old_ptrs
    ema.update()
    for k, e, s in zip(ema.names, ema.shadows, shadows):
        torch.testing.assert_close(e, s + 0.5 * (new[k] - s), rtol=1e-6, atol=1e-7, msg=lambda m: f"{k}: {m}")
    with ema.applied():
        for k, e in zip(ema.names, ema.shadows):
            assert torch.equal(e, new[k]), k  # the exchange reached the new tensors too
    assert all(torch.equal(v, new[k]) for k, v in model.state_dict().items())


def test_a_host_side_skip_flag_is_honoured():
    model = _tiny()
    ema = EMA(model, decay=0.5)
    start = [e.clone() for e in ema.shadows]
    _perturb(model, 12)
    ema.update(skip_if_nonzero=torch.ones(1))
    assert all(torch.equal(e, s) for e, s in zip(ema.shadows, start)) and ema.num_updates == 1
    ema.undo_update_count()
    ema.update(skip_if_nonzero=torch.zeros(1))
    assert any(not torch.equal(e, s) for e, s in zip(ema.shadows, start)) and ema.num_updates == 1


def test_train_one_epoch_updates_after_every_step():
    model = _tiny()
    twin = _tiny()
    ema = EMA(model, decay=0.9)
    batches = _batches(3)
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    seg_amd.train_one_epoch(model, batches, nn.CrossEntropyLoss(), opt, "cpu", progress=False, ema=ema)
    assert ema.num_updates == 3
    # the same run by hand: a torch lerp after every step
    opt2 = torch.optim.SGD(twin.parameters(), lr=1e-2)
    ref = {k: v.clone() for k, v in twin.state_dict().items() if v.is_floating_point()}
    for b in batches:
        seg_amd.train_one_epoch(twin, [b], nn.CrossEntropyLoss(), opt2, "cpu", progress=False)
        for k, v in twin.state_dict().items():
            if k in ref:
                ref[k].lerp_(v, 1.0 - 0.9)
    for k, e in zip(ema.names, ema.shadows):
        assert torch.equal(e, ref[k]), k
    for k, v in model.state_dict().items():
        assert torch.equal(v, twin.state_dict()[k]), k  # the average never touches the run


def test_out_of_range_label_on_cpu_leaves_the_average_alone():
    model = _tiny()
    ema = EMA(model, decay=0.9)
    x, y = _batches(1)[0]
    y = y.clone()
    y[0, 0, 0] = 4
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    start = [e.clone() for e in ema.shadows]
    with pytest.raises((IndexError, RuntimeError)):
        seg_amd.train_one_epoch(model, [(x, y)], nn.CrossEntropyLoss(), opt, "cpu", progress=False, ema=ema)
    assert ema.num_updates == 0 and all(torch.equal(e, s) for e, s in zip(ema.shadows, start))


def test_train_model_validates_and_saves_the_averaged_weights(tmp_path, capsys, monkeypatch):
    model = _tiny()
    ema = EMA(model, decay=0.9)
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    val_loader = _batches(2, seed0=7)
    seen = []
    real_validate = seg_amd.train.validate

    def spy_validate(m, *a, **k):
        seen.append({k2: v.clone() for k2, v in getattr(m, "module", m).state_dict().items()})
        return real_validate(m, *a, **k)

    monkeypatch.setattr(seg_amd.train, "validate", spy_validate)
    best = str(tmp_path / "best.pth")
    train_model(model, _batches(2), nn.CrossEntropyLoss(), opt, "cpu", epochs=1,
                checkpoint_pattern=str(tmp_path / "e_{epoch}.pth"), progress=False, val_loader=val_loader,
                best_checkpoint=best, ema=ema, ema_checkpoint_pattern=str(tmp_path / "ema_{epoch}.pth"))
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("EMA of the weights (decay 0.9)") and "averaged weights" in out[0]
    assert ema.num_updates == 2 and model.training
    avg, live = ema.averaged_state_dict(), model.state_dict()
    assert any(not torch.equal(avg[k], live[k]) for k in ema.names)
    assert sorted(os.listdir(tmp_path)) == ["best.pth", "e_1.pth", "ema_1.pth"]
    for name, want in (("best.pth", avg), ("ema_1.pth", avg), ("e_1.pth", live)):
        sd = torch.load(tmp_path / name)
        assert list(sd) == list(want), name
        for k in want:
            assert torch.equal(sd[k], want[k]), (name, k)
    assert len(seen) == 1 and all(torch.equal(seen[0][k], avg[k]) for k in avg)  # validation ran on the average
    want = real_validate(_loaded(avg), val_loader, nn.CrossEntropyLoss(), "cpu", progress=False)["loss"]
    assert f"  Validation Loss: {want:.4f}" in out


def _loaded(sd):
    m = _tiny(seed=5)
    m.load_state_dict(sd, strict=True)
    return m


def test_train_model_without_ema_prints_and_saves_as_before(tmp_path, capsys):
    model = _tiny()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    train_model(model, _batches(1), nn.CrossEntropyLoss(), opt, "cpu", epochs=1,
                checkpoint_pattern=str(tmp_path / "e_{epoch}.pth"), progress=False)
    out = capsys.readouterr().out
    assert "EMA" not in out and os.listdir(tmp_path) == ["e_1.pth"]
