"""CPU: the validation surface -- seg_amd.metrics.summarize, seg_amd.validate on the torch
composition (the same code path as on the MI355X, with `forward_metrics` running in torch
ops), train_model(val_loader=..., best_checkpoint=...), and the sharded evaluation over gloo.
"""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F
from torch import nn

import seg_amd
from seg_amd import UNet, deterministic_init, summarize, synthetic_batch, train_model, validate
from seg_amd.detinit import miou


# ------------------------------------------------------------------------------ summarize
def test_summarize_hand_made():
    cm = torch.tensor([[5, 1, 0],
                       [2, 3, 0],
                       [0, 0, 0]])  # class 2: never a label, never predicted -> empty union
    s = summarize(cm)
    assert s["confusion"].dtype == torch.int64 and s["confusion"].device.type == "cpu"
    assert torch.equal(s["confusion"], cm)
    assert s["pixel_acc"] == 8 / 11
    assert s["iou"][0].item() == 5 / 8 and s["iou"][1].item() == 3 / 6 and math.isnan(s["iou"][2].item())
    assert s["miou"] == pytest.approx((5 / 8 + 3 / 6) / 2, abs=1e-15)
    # a class that is predicted but never a label has a union: IoU 0, and it counts
    s = summarize(torch.tensor([[4, 2], [0, 0]]))
    assert s["iou"].tolist() == [4 / 6, 0.0] and s["miou"] == pytest.approx(2 / 6, abs=1e-15)
    # nothing counted at all
    s = summarize(torch.zeros(3, 3, dtype=torch.int64))
    assert math.isnan(s["miou"]) and math.isnan(s["pixel_acc"]) and s["iou"].isnan().all()


def test_summarize_agrees_with_detinit_miou():
    g = torch.Generator().manual_seed(0)
    C = 6
    target = torch.randint(0, C - 1, (3, 16, 20), generator=g)  # class 5 absent from the labels
    pred = torch.randint(0, C - 2, (3, 16, 20), generator=g)    # classes 4, 5 never predicted
    cm = torch.bincount((target * C + pred).reshape(-1), minlength=C * C).reshape(C, C)
    s = summarize(cm)
    assert s["miou"] == pytest.approx(miou(pred, target, C), abs=1e-15)
    assert math.isnan(s["iou"][5].item()) and s["iou"][4].item() == 0.0
    assert s["pixel_acc"] == pytest.approx((pred == target).double().mean().item(), abs=1e-15)


# ------------------------------------------------------------------------------- validate
def _tiny(seed=1):
    return deterministic_init(UNet(4, 8), seed=seed)


def _shards(n, seed0=0):
    out = []
    for k in range(n):
        x, y = synthetic_batch(2, 32, 64, 4, seed=seed0 + k)
        y[0, k % 32, :5] = -100
        out.append((x, y))
    return out


def _direct(model, loader, ignore_index=-100):
    """The plain torch computation validate() must reproduce (eval mode, no gradients)."""
    model.eval()
    C = 4
    cm = torch.zeros(C, C, dtype=torch.int64)
    total = 0.0
    with torch.no_grad():
        for x, y in loader:
            logits = model(x)
            total += F.cross_entropy(logits, y, ignore_index=ignore_index).item()
            keep = y != ignore_index
            cm += torch.bincount(y[keep] * C + logits.argmax(1)[keep], minlength=C * C).reshape(C, C)
    return total / len(loader), cm


def _same_summary(a, b):
    assert torch.equal(a["confusion"], b["confusion"])
    assert a["pixel_acc"] == b["pixel_acc"]
    assert torch.equal(a["iou"].nan_to_num(-1), b["iou"].nan_to_num(-1))
    assert a["miou"] == b["miou"] or (math.isnan(a["miou"]) and math.isnan(b["miou"]))


@pytest.mark.parametrize("criterion", [nn.CrossEntropyLoss(), nn.CrossEntropyLoss(label_smoothing=0.1)],
                         ids=["fused-surface", "fallback"])
def test_validate_cpu_matches_direct_torch(criterion):
    model = _tiny().train()
    loader = _shards(3)
    out = validate(model, loader, criterion, "cpu", progress=False)
    assert model.training, "validate() must restore the caller's mode"
    want_loss, cm = _direct(_tiny(), loader)
    if criterion.label_smoothing:
        m = _tiny().eval()
        with torch.no_grad():
            want_loss = sum(criterion(m(x), y).item() for x, y in loader) / len(loader)
    assert out["loss"] == pytest.approx(want_loss, rel=1e-12)
    _same_summary(out, summarize(cm))
    assert set(out) == {"loss", "confusion", "pixel_acc", "iou", "miou"}
    model.eval()
    validate(model, loader, criterion, "cpu", progress=False)
    assert not model.training


def test_validate_takes_ignore_index_from_the_criterion():
    model = _tiny()
    loader = [(x, torch.where(y == -100, torch.full_like(y, 255), y)) for x, y in _shards(2)]
    out = validate(model, loader, nn.CrossEntropyLoss(ignore_index=255), "cpu", progress=False)
    want_loss, cm = _direct(_tiny(), loader, ignore_index=255)
    assert out["loss"] == pytest.approx(want_loss, rel=1e-12)
    assert torch.equal(out["confusion"], cm) and int(cm.sum()) == 2 * 2 * 32 * 64 - 2 * 5


def test_forward_metrics_cpu_accumulates_and_raises_on_bad_label():
    model = _tiny().eval()
    x, y = _shards(1)[0]
    cm = torch.zeros(4, 4, dtype=torch.int64)
    loss = model.forward_metrics(x, y, cm)
    once = cm.clone()
    model.forward_metrics(x, y, cm)
    assert torch.equal(cm, 2 * once) and not loss.requires_grad
    twin = seg_amd.traceable(model)
    cm2 = torch.zeros(4, 4, dtype=torch.int64)
    assert twin.forward_metrics(x, y, cm2).item() == loss.item() and torch.equal(cm2, once)
    y[1, 3, 3] = 4
    with pytest.raises((IndexError, RuntimeError)):
        validate(model, [(x, y)], nn.CrossEntropyLoss(), "cpu", progress=False)


# ---------------------------------------------------------------------------- train_model
def test_train_model_without_val_loader_is_unchanged(tmp_path, capsys):
    model = _tiny()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    pattern = str(tmp_path / "ck" / "e_{epoch}.pth")
    seen = []
    orig = seg_amd.train.train_one_epoch
    try:
        seg_amd.train.train_one_epoch = lambda *a, **k: seen.append(orig(*a, **k)) or seen[-1]
        train_model(model, _shards(2), nn.CrossEntropyLoss(), opt, "cpu", epochs=2, checkpoint_pattern=pattern,
                    progress=False)
    finally:
        seg_amd.train.train_one_epoch = orig
    out = capsys.readouterr().out
    assert out == (f"  Training Loss: {seen[0]:.4f}\n  Training Loss: {seen[1]:.4f}\n"
                   "Training completed. Best validation loss: inf\n")
    assert sorted(os.listdir(tmp_path / "ck")) == ["e_1.pth", "e_2.pth"]
    assert sorted(os.listdir(tmp_path)) == ["ck"]
    sd = torch.load(tmp_path / "ck" / "e_2.pth")
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())


def test_train_model_with_val_loader_prints_and_saves_best(tmp_path, capsys, monkeypatch):
    """Scripted validation losses 0.5, 0.7, 0.3: the best checkpoint is written after epochs 1 and
    3 only, the per-epoch checkpoints stay, and the lines are the reference's."""
    model = _tiny()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    val_loader = _shards(1, seed0=7)
    script = iter([0.5, 0.7, 0.3])
    calls = []

    def fake_validate(m, loader, criterion, device, progress=True, epoch=0, epochs=1):
        assert loader is val_loader
        calls.append((epoch, epochs))
        return {"loss": next(script)}

    saves = []
    real_save = torch.save

    def spy_save(obj, path, *a, **k):
        saves.append(os.path.relpath(str(path), str(tmp_path)))
        return real_save(obj, path, *a, **k)

    monkeypatch.setattr(seg_amd.train, "validate", fake_validate)
    monkeypatch.setattr(torch, "save", spy_save)
    train_losses = []
    orig = seg_amd.train.train_one_epoch
    monkeypatch.setattr(seg_amd.train, "train_one_epoch",
                        lambda *a, **k: train_losses.append(orig(*a, **k)) or train_losses[-1])
    best = str(tmp_path / "best" / "best.pth")
    train_model(model, _shards(2), nn.CrossEntropyLoss(), opt, "cpu", epochs=3,
                checkpoint_pattern=str(tmp_path / "e_{epoch}.pth"), progress=False, val_loader=val_loader,
                best_checkpoint=best)
    out = capsys.readouterr().out
    t = [f"{v:.4f}" for v in train_losses]
    assert out == (f"\nEpoch 1/3:\n  Training Loss: {t[0]}\n  Validation Loss: 0.5000\n"
                   "  Validation loss improved! Saving model...\n"
                   f"\nEpoch 2/3:\n  Training Loss: {t[1]}\n  Validation Loss: 0.7000\n"
                   f"\nEpoch 3/3:\n  Training Loss: {t[2]}\n  Validation Loss: 0.3000\n"
                   "  Validation loss improved! Saving model...\n"
                   "Training completed. Best validation loss: 0.3000\n")
    assert calls == [(0, 3), (1, 3), (2, 3)]
    assert saves == ["best/best.pth", "e_1.pth", "e_2.pth", "best/best.pth", "e_3.pth"]
    sd = torch.load(best)
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())


def test_train_model_with_real_validation(tmp_path, capsys):
    model = _tiny()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    val_loader = _shards(2, seed0=7)
    train_model(model, _shards(2), nn.CrossEntropyLoss(), opt, "cpu", epochs=1, checkpoint_pattern=None,
                progress=False, val_loader=val_loader, best_checkpoint=str(tmp_path / "best.pth"))
    assert model.training  # validate() handed the training mode back
    out = capsys.readouterr().out.splitlines()
    want = validate(model, val_loader, nn.CrossEntropyLoss(), "cpu", progress=False)["loss"]
    assert out[0] == "" and out[1] == "Epoch 1/1:" and out[2].startswith("  Training Loss: ")
    assert out[3:] == [f"  Validation Loss: {want:.4f}", "  Validation loss improved! Saving model...",
                       f"Training completed. Best validation loss: {want:.4f}"]
    assert os.listdir(tmp_path) == ["best.pth"]


# -------------------------------------------------------------------------- gloo, world 2
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _val_worker(rank, world, port, results):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from seg_amd.ddp import DataParallel
        model = deterministic_init(UNet(4, 8), seed=50 + rank)  # the wrapper's broadcast makes them equal
        dp = DataParallel(model)
        shard = _shards(2, seed0=20 + 10 * rank)  # different data per rank
        out = validate(dp, shard, nn.CrossEntropyLoss(), "cpu", progress=False)
        plain = validate(model, shard, nn.CrossEntropyLoss(label_smoothing=0.1), "cpu", progress=False)
        results[rank] = (out, plain)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_validate_sharded_over_gloo():
    world = 2
    mgr = mp.Manager()
    results = mgr.dict()
    mp.spawn(_val_worker, args=(world, _free_port(), results), nprocs=world, join=True)
    (a, pa), (b, pb) = results[0], results[1]
    single = deterministic_init(UNet(4, 8), seed=50)
    both = _shards(2, seed0=20) + _shards(2, seed0=30)
    want = validate(single, both, nn.CrossEntropyLoss(), "cpu", progress=False)
    for got in (a, b):
        assert got["loss"] == pytest.approx(want["loss"], rel=1e-12)
        _same_summary(got, want)
    assert a["loss"] == b["loss"]
    # without the wrapper (the default group) and with an unfusable criterion: still one result on both ranks
    assert pa["loss"] == pb["loss"] and torch.equal(pa["confusion"], pb["confusion"])
    assert torch.equal(pa["confusion"], want["confusion"])
