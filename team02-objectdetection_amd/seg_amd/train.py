"""Drop-in training loop: `train_model(model, train_loader, criterion, optimizer,
device, epochs=10)` with the reference's signature and behaviour
(src/train.py:6-79): per epoch `model.train()`, for each batch `.to(device)`,
`optimizer.zero_grad()`, forward, `criterion`, `backward`, `optimizer.step()`,
running loss, a per-epoch "Training Loss" line and a state_dict checkpoint
`Models/obj/obj_MOB_1_epoch_{epoch}.pth` (src/train.py:77).

MI355X differences (results are the same):
  * when `criterion` is an `nn.CrossEntropyLoss` (main.py:99; class weights,
    label smoothing and reduction "mean" / "sum" included) or a `seg_amd.SegLoss`
    (focal exponent and soft Dice term) or a `seg_amd.OhemCELoss` (online hard
    example mining) or a `seg_amd.DistillLoss` (knowledge distillation from a
    seg_amd teacher, whose logits are upsampled inside the same kernels) and the model is a
    seg_amd model, the loss is computed by the fused upsample+cross-entropy
    kernels (`model.forward_loss`), so the 168 MB of full-resolution logits
    per bs=32 batch are never written;
  * `max_grad_norm` (not in the reference) clips the gradients' global L2 norm before
    every step; with seg_amd.Adam / seg_amd.AdamW / seg_amd.SGD the coefficient stays on the
    device and is applied inside the step (seg_amd/optim.py);
  * `scheduler` (not in the reference) is a learning-rate scheduler stepped after every
    optimizer step, or once per epoch (seg_amd.PolyLR, torch.optim.lr_scheduler.*);
  * `ema` (not in the reference) keeps an exponential moving average of the weights, one launch
    after every step; validation and `best_checkpoint` then use the averaged model (seg_amd/ema.py);
  * under torch.distributed the gradients are averaged across ranks by
    seg_amd.ddp (RCCL all-reduce overlapped with the backward) and only
    rank 0 prints and writes checkpoints.
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch
from torch import nn

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    tqdm = None


def fused_loss_options(criterion):
    """The keyword arguments of model.forward_loss / forward_metrics that reproduce `criterion`, or
    None when it has to run on the full-resolution logits: anything but an nn.CrossEntropyLoss
    (a subclass with a forward of its own included), and reduction="none", whose result is a
    full-resolution tensor.  A seg_amd.SegLoss (again without a forward of its own) adds its four
    scalars: ce, dice, focal_gamma and dice_smooth; a seg_amd.OhemCELoss (the same rule) its two: ohem_thresh and
    ohem_min_kept; a seg_amd.DistillLoss (the same rule) ce, kd, kd_temperature and kd_ignored -- the teacher's
    logits are compute_loss's to add.  A seg_amd.BinarySegLoss (the same rule) gives binary=True with its bce
    coefficient as ce, and dice, focal_gamma, dice_smooth and pos_weight; its threshold is validation's to add."""
    from .losses import BinarySegLoss, DistillLoss, OhemCELoss, SegLoss
    if isinstance(criterion, BinarySegLoss):
        if type(criterion).forward is not BinarySegLoss.forward:
            return None
        return {"ignore_index": criterion.ignore_index, "binary": True, "ce": float(criterion.bce),
                "dice": float(criterion.dice), "focal_gamma": float(criterion.focal_gamma),
                "dice_smooth": float(criterion.dice_smooth), "pos_weight": float(criterion.pos_weight)}
    if isinstance(criterion, DistillLoss):
        if type(criterion).forward is not DistillLoss.forward:
            return None
        return {"ignore_index": criterion.ignore_index, "weight": criterion.weight, "label_smoothing": 0.0,
                "reduction": "mean", "ce": float(criterion.ce), "kd": float(criterion.kd),
                "kd_temperature": float(criterion.temperature), "kd_ignored": bool(criterion.kd_ignored)}
    if isinstance(criterion, OhemCELoss):
        if type(criterion).forward is not OhemCELoss.forward:
            return None
        return {"ignore_index": criterion.ignore_index, "weight": criterion.weight, "label_smoothing": 0.0,
                "reduction": "mean", "ohem_thresh": float(criterion.thresh), "ohem_min_kept": criterion.min_kept}
    if isinstance(criterion, SegLoss):
        if type(criterion).forward is not SegLoss.forward:
            return None
        return {"ignore_index": criterion.ignore_index, "weight": criterion.weight,
                "label_smoothing": float(criterion.label_smoothing), "reduction": "mean",
                "ce": float(criterion.ce), "dice": float(criterion.dice),
                "focal_gamma": float(criterion.focal_gamma), "dice_smooth": float(criterion.dice_smooth)}
    if not isinstance(criterion, nn.CrossEntropyLoss) or type(criterion).forward is not nn.CrossEntropyLoss.forward:
        return None
    if criterion.reduction not in ("mean", "sum"):
        return None
    return {"ignore_index": criterion.ignore_index, "weight": criterion.weight,
            "label_smoothing": float(criterion.label_smoothing), "reduction": criterion.reduction}


def _is_rank0() -> bool:
    return not (torch.distributed.is_available() and torch.distributed.is_initialized()) or \
        torch.distributed.get_rank() == 0


def _raise_bad_labels(n: float):
    if n:
        raise IndexError("Target out of bounds: label(s) outside [0, num_classes) that are not ignore_index "
                         "(nn.CrossEntropyLoss raises on these; the optimizer step was skipped)")


def _check_labels(model, inputs):
    """Raise IndexError like nn.CrossEntropyLoss if the fused loss saw a label outside
    [0, C) (the kernels flag it; the loss and gradients are NaN), BEFORE optimizer.step():
    the path for optimizers that cannot skip their step on the device.  Under
    seg_amd.ddp.DataParallel the count arrived with the last gradient bucket's all-reduce
    (every rank raises together, no extra collective).  When it did not (a no_sync step, or
    another wrapper under torch.distributed) the counts are summed over the ranks by an
    all-reduce of their own, so a peer never blocks in the next collective; in one
    process it was copied to the host right after the loss kernel, so this waits for the
    forward only."""
    if not inputs.is_cuda:
        return  # the CPU composition's F.cross_entropy raises by itself
    from .engine import bad_label_count, bad_label_count_host, label_flag
    if hasattr(model, "label_flag"):
        flag = label_flag(model)
        if flag is not None:
            _raise_bad_labels(float(flag.item()))
            return
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        bad = bad_label_count(model)
        bad = torch.zeros(1, dtype=torch.float32, device=inputs.device) if bad is None else bad
        torch.distributed.all_reduce(bad)
        _raise_bad_labels(float(bad.item()))
        return
    n = bad_label_count_host(model)
    _raise_bad_labels(n or 0)


def _step_and_loss(model, inputs, optimizer, loss, max_grad_norm=None, ema=None):
    """optimizer.step() and loss.item() (src/train.py:39-41) with the fused loss's label check.  With seg_amd.Adam,
    seg_amd.AdamW or seg_amd.SGD the step is queued at once and skips itself on the device when the batch (on any
    rank) had an out-of-range label; the host reads the flag after loss.item(), whose wait covers it, and raises --
    no host wait before the step and no extra collective.  Other optimizers: the check runs
    before the step.

    max_grad_norm: clip the global L2 norm of the gradients of the optimizer's parameters (after
    finish_gradient_sync they are the averaged ones, the same on every rank: no collective).  The seg_amd
    optimizers take the coefficient of seg_amd.grad_norm as the step's grad_scale -- nothing waits and .grad stays
    unclipped; any other optimizer gets seg_amd.clip_grad_norm_ in place, after the label check.

    ema: a seg_amd.EMA over the same model, updated right after the step.  Behind a step that skips itself on the
    device it gets the same flag (a skipped step is not averaged in, still without a host wait) and its update count
    goes back with the optimizer's before the loop raises; behind a host-side label check it is a plain update()."""
    from .optim import SGD, Adam, AdamW, clip_grad_norm_, grad_norm
    from .engine import label_flag
    flag = label_flag(model) if inputs.is_cuda else None
    ours = isinstance(optimizer, (Adam, AdamW, SGD))
    scale = None
    if max_grad_norm is not None:
        params = [p for group in optimizer.param_groups for p in group["params"]]
        if ours and inputs.is_cuda:
            scale = {"grad_scale": grad_norm(params, max_grad_norm)[1:2]}
    if flag is None or not ours:
        _check_labels(model, inputs)
        if scale is not None:
            optimizer.step(**scale)
        else:
            if max_grad_norm is not None:
                clip_grad_norm_(params, max_grad_norm)
            optimizer.step()
        if ema is not None:
            ema.update()
        return loss.item()
    core = getattr(model, "module", model)
    host = core.__dict__.get("_segamd_flag_host")
    if host is None:
        host = core.__dict__["_segamd_flag_host"] = torch.zeros(1, dtype=torch.float32).pin_memory()
    host.copy_(flag, non_blocking=True)  # stream-ordered before the step and the loss copy below
    optimizer.step(skip_if_nonzero=flag, **(scale or {}))
    if ema is not None:
        ema.update(skip_if_nonzero=flag)  # the same flag: a skipped step is not averaged in
    lv = loss.item()                     # waits for this stream: the flag copy has landed
    if float(host[0]):
        optimizer.undo_step_count()      # the device skipped the step: its counters go back too
        if ema is not None:
            ema.undo_update_count()
        _raise_bad_labels(float(host[0]))
    return lv


def compute_loss(model, criterion, inputs, targets):
    """criterion(model(inputs), targets), fused when the pair allows it.  A seg_amd.DistillLoss is fused when both
    models are seg_amd models on the GPU: the teacher's forward_low_logits(inputs) goes to the student's forward_loss
    as teacher_logits and neither model's full-resolution logits are formed; otherwise it is
    criterion(model(inputs), targets, criterion.teacher_logits(inputs))."""
    from .losses import DistillLoss
    core = getattr(model, "module", model)
    opts = fused_loss_options(criterion) if hasattr(core, "forward_loss") else None
    if isinstance(criterion, DistillLoss):
        teacher = getattr(criterion.teacher, "module", criterion.teacher)
        if opts is not None and inputs.is_cuda and hasattr(teacher, "forward_low_logits"):
            if teacher.training:
                raise RuntimeError("DistillLoss: the teacher is in training mode; call teacher.eval()")
            return model.forward_loss(inputs, targets, teacher_logits=teacher.forward_low_logits(inputs), **opts)
        return criterion(model(inputs), targets, criterion.teacher_logits(inputs))
    if opts is not None:
        return model.forward_loss(inputs, targets, **opts)
    return criterion(model(inputs), targets)


def train_one_epoch(model, train_loader, criterion, optimizer, device, epoch: int = 0, epochs: int = 1,
                    progress: bool = True, augment=None, max_grad_norm: float | None = None, ema=None,
                    scheduler=None) -> float:
    """One pass over `train_loader`; returns the mean batch loss (src/train.py:31-44).

    max_grad_norm: clip the gradients' global L2 norm to it before every step (_step_and_loss); None: no clipping.

    ema: a seg_amd.EMA built over `model`: updated after every optimizer step (one launch, no host wait; a step
    skipped for an out-of-range label is not averaged in).

    scheduler: a learning-rate scheduler over `optimizer` (seg_amd.PolyLR, torch.optim.lr_scheduler.*): its step()
    is called after every optimizer step.  A batch whose step was skipped for an out-of-range label raises before
    the scheduler is touched.

    augment: optional seg_amd.augment.GpuAugment -- the loader then yields decoded
    uint8 batches (images [N,Hs,Ws,3] RGB, masks [N,Hs,Ws] raw class ids) and the
    readers' albumentations pipeline runs on the GPU."""
    model.train()
    train_loss = 0.0
    it = train_loader
    bar = None
    if progress and tqdm is not None and _is_rank0():
        bar = it = tqdm(train_loader, desc=f"Epoch {epoch + 1}/{epochs} [Train]", leave=True, position=0,
                        bar_format="{l_bar}{bar:20}{r_bar}{bar:-20b}")
    nb = 0
    for inputs, targets in it:
        inputs = inputs.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        if augment is not None:  # per-(rank, epoch, batch) parameter stream
            rank = torch.distributed.get_rank() if not _is_rank0() else 0
            rng = np.random.Generator(np.random.PCG64([rank, epoch, nb]))
            inputs, targets = augment(inputs, targets, rng=rng)
        optimizer.zero_grad()
        loss = compute_loss(model, criterion, inputs, targets)
        loss.backward()
        sync = getattr(model, "finish_gradient_sync", None)
        if sync is not None:
            sync()
        # the update never sees an out-of-range label's NaN gradients, on any rank (nn.CrossEntropyLoss raises in
        # the forward): seg_amd.Adam skips its step on the device, everything else is checked before the step
        lv = _step_and_loss(model, inputs, optimizer, loss, max_grad_norm, ema)
        if scheduler is not None:
            scheduler.step()
        train_loss += lv
        nb += 1
        if bar is not None:
            bar.set_postfix(loss=f"{lv:.4f}")
    n = len(train_loader) if hasattr(train_loader, "__len__") else max(nb, 1)
    return train_loss / max(n, 1)


def _num_classes(core) -> int:
    """Output channels of a segmentation model: its last convolution's (outc / sem_out heads)."""
    convs = [m for m in core.modules() if isinstance(m, nn.Conv2d)]
    if not convs:
        raise ValueError("validate(): cannot tell the number of classes of a model without convolutions")
    return convs[-1].out_channels


def tta_loss_options(criterion):
    """The hard term of `criterion` as forward_metrics_tta's keyword arguments: class weights, ignore_index and
    reduction ("mean" unless an nn.CrossEntropyLoss asks for "sum").  Label smoothing, Dice, focal and OHEM terms
    shape training, not an ensemble's report, and are left out -- the rule validate() already applies to a
    DistillLoss.  ValueError for a criterion that is none of the fused ones (fused_loss_options)."""
    if fused_loss_options(criterion) is None:
        raise ValueError("validate(tta=...) takes an nn.CrossEntropyLoss (reduction 'mean' or 'sum'), a seg_amd.SegLoss, "
                         f"OhemCELoss or DistillLoss, got {type(criterion).__name__}")
    reduction = criterion.reduction if isinstance(criterion, nn.CrossEntropyLoss) else "mean"
    return {"ignore_index": criterion.ignore_index, "weight": criterion.weight, "reduction": reduction}


def validate(model, val_loader, criterion, device, progress: bool = True, epoch: int = 0, epochs: int = 1,
             tta=None) -> dict:
    """One pass over `val_loader` in eval mode, without gradients: the reference's disabled
    validation phase (src/train.py:46-66) plus the metrics of seg_amd.metrics.summarize.

    Returns {"loss": mean of the batch means (val_loss += loss.item(); / len(val_loader)),
    "confusion", "pixel_acc", "iou", "miou"}.  The previous train/eval mode is restored.

    When `criterion` is an nn.CrossEntropyLoss, a seg_amd.SegLoss or a seg_amd.OhemCELoss (fused_loss_options: class weights, label
    smoothing, reduction "mean" / "sum", Dice and focal terms included -- they change "loss" only, never the
    matrix) and the
    model has `forward_metrics`, each batch is one fused forward (loss + argmax + confusion matrix
    from the low-resolution logits); any other pair runs criterion(model(x), t) with argmax and bincount on the
    device.  Either way the batch losses and the matrix stay on the device and the host waits
    once, at the end of the pass -- so the bar shows no per-batch loss.  An out-of-range label
    raises IndexError there.  Under torch.distributed every rank evaluates its own shard; the
    matrices and [sum of batch losses, #batches, #bad labels] are summed with one all-reduce each
    (on the wrapper's process group when the model has one) and every rank returns the same dict.

    A seg_amd.DistillLoss is evaluated as its hard() term, nn.CrossEntropyLoss(weight, ignore_index): the student's
    validation loss is a hard-label quantity (train_model's best_checkpoint compares it) and no teacher forward
    runs.

    tta (a seg_amd.TTA, or "hflip"): every batch is evaluated as a test-time-augmentation ensemble,
    model.forward_metrics_tta (seg_amd/tta.py has the definition): loss = NLLLoss(log p) of the averaged class
    probabilities, the matrix from their argmax.  Any fused criterion is then evaluated as its HARD term -- class
    weights, ignore_index, reduction (tta_loss_options): label smoothing, Dice, focal and OHEM terms shape training,
    not an ensemble's report.  Everything else -- the one host wait, the IndexError, the two all-reduces -- is as
    without it; tta=None runs every line of the path above as it always did.

    A seg_amd.BinarySegLoss (one-logit model): the matrix is [2, 2], confusion[label, z > zthr] with
    zthr = log(threshold / (1 - threshold)) of the criterion's threshold (strict: a tie is background), on the fused
    branch (seg_bce_upsample_eval) and on the unfused one (logits[:, 0] > zthr, not argmax) alike; the dict
    additionally holds "precision", "recall" and "f1" of class 1 (seg_amd.metrics.binary_summary).  With tta= it is a
    ValueError."""
    from .losses import BinarySegLoss, DistillLoss, binary_target, logit_threshold
    from .metrics import add_confusion, binary_summary, summarize
    if isinstance(criterion, DistillLoss):
        criterion = criterion.hard()  # validation does not distil: hard-label loss and mIoU, no teacher forward
    core = getattr(model, "module", model)
    ignore_index = getattr(criterion, "ignore_index", -100)
    binary = isinstance(criterion, BinarySegLoss)
    if binary and tta is not None:
        raise ValueError("validate(tta=...) is not defined for a BinarySegLoss: an ensemble of a one-logit model is "
                         "out of scope")
    if tta is not None:
        from .tta import as_tta
        tta = as_tta(tta)
        if not hasattr(core, "forward_metrics_tta"):
            raise ValueError(f"validate(tta=...) needs a seg_amd model, got {type(core).__name__}")
        opts = tta_loss_options(criterion)
    else:
        opts = fused_loss_options(criterion) if hasattr(core, "forward_metrics") else None
        if binary and opts is not None:
            opts["threshold"] = float(criterion.threshold)
    fused = opts is not None
    it = val_loader
    if progress and tqdm is not None and _is_rank0():
        it = tqdm(val_loader, desc=f"Epoch {epoch + 1}/{epochs} [Valid]", leave=True, position=0,
                  bar_format="{l_bar}{bar:20}{r_bar}{bar:-20b}")
    was_training = model.training
    model.eval()
    confusion = acc = None  # acc (float64): sum of batch losses, #batches, #out-of-range labels
    try:
        with torch.no_grad():
            for inputs, targets in it:
                inputs = inputs.to(device, non_blocking=True)
                targets = targets.to(device, non_blocking=True)
                if acc is None:
                    acc = torch.zeros(3, dtype=torch.float64, device=inputs.device)
                if fused:
                    if confusion is None:
                        C = 2 if binary else _num_classes(core)
                        confusion = torch.zeros((C, C), dtype=torch.int64, device=inputs.device)
                    if tta is not None:
                        loss = model.forward_metrics_tta(inputs, targets, confusion, tta, **opts)
                    else:
                        loss = model.forward_metrics(inputs, targets, confusion, **opts)
                    if inputs.is_cuda:  # the CPU composition's F.cross_entropy raises by itself
                        from .engine import bad_label_count
                        acc[2] += bad_label_count(model)[0]
                else:
                    logits = model(inputs)
                    loss = criterion(logits, targets)
                    if confusion is None:
                        C = 2 if binary else logits.shape[1]
                        confusion = torch.zeros((C, C), dtype=torch.int64, device=inputs.device)
                    if binary:  # the criterion's threshold on the one logit, strictly: never argmax
                        pred = (logits[:, 0] > logit_threshold(criterion.threshold)).to(torch.int64)
                        add_confusion(confusion, pred, binary_target(logits, targets), ignore_index)
                    else:
                        add_confusion(confusion, logits.argmax(1), targets, ignore_index)
                acc[0] += loss.detach().double()
                acc[1] += 1
    finally:
        model.train(was_training)
    if acc is None:
        raise ValueError("validate(): the validation loader yielded no batch")
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        pg = getattr(model, "pg", None)
        torch.distributed.all_reduce(confusion, group=pg)
        torch.distributed.all_reduce(acc, group=pg)
    # the pass's only host wait: one copy carries the matrix and the three float64 sums (as their bit patterns)
    host = torch.cat([confusion.reshape(-1), acc.view(torch.int64)]).cpu()
    loss_sum, nb, bad = host[-3:].view(torch.float64).tolist()
    if bad:
        raise IndexError(f"Target out of bounds: {int(bad)} label(s) outside [0, num_classes) that are not "
                         "ignore_index (nn.CrossEntropyLoss raises on these)")
    out = {"loss": loss_sum / nb}
    out.update(summarize(host[:-3].reshape(confusion.shape)))
    if binary:
        out.update(binary_summary(out["confusion"]))
    return out


def train_model(model, train_loader, criterion, optimizer, device, epochs=10,
                checkpoint_pattern: str | None = "Models/obj/obj_MOB_1_epoch_{epoch}.pth", progress: bool = True,
                augment=None, val_loader=None, best_checkpoint: str | None = None, freeze=None,
                freeze_epochs: int | None = None, max_grad_norm: float | None = None, ema=None,
                ema_checkpoint_pattern: str | None = None, val_tta=None, scheduler=None,
                scheduler_interval: str = "step"):
    """Train for `epochs` epochs (src/train.py:6-79).  With `val_loader`, each epoch ends with the
    reference's validation phase (commented out there, src/train.py:46-76): validate(), the
    epoch's result lines, and on an improved validation loss a state_dict at `best_checkpoint`
    (when given).  Without it, output and files are the reference's as it stands.

    freeze: what seg_amd.freeze takes ("backbone", a module, a list of either) -- frozen (parameters and
    BatchNorm statistics) before the first epoch; freeze_epochs=K unfreezes it before epoch K+1, None keeps it
    frozen for the whole run.  One line is printed at each change; without `freeze` nothing changes.

    max_grad_norm: train_one_epoch's -- the gradients' global L2 norm is clipped to it before every step.

    ema: a seg_amd.EMA built over the same model, updated after every step.  With it the per-epoch validation runs
    on the averaged weights (under ema.applied(): the model's own plans, no copy) and `best_checkpoint` receives
    ema.averaged_state_dict(); `ema_checkpoint_pattern` (formatted like `checkpoint_pattern`), if given, receives
    the averaged weights every epoch.  `checkpoint_pattern`'s file keeps the live weights.  Under DataParallel every
    rank keeps its own EMA (averaged gradients and broadcast BatchNorm statistics keep them equal without a
    collective) and rank 0 writes the files.  One line at the start says which weights validation uses.

    val_tta: validate()'s tta -- the per-epoch validation (and so best_checkpoint's comparison) evaluates the
    flip / multi-scale ensemble; with `ema` it is the ensemble of the averaged weights.

    scheduler: a learning-rate scheduler over `optimizer`; scheduler_interval="step" (default) steps it after every
    optimizer step (train_one_epoch's scheduler -- a per-iteration schedule such as seg_amd.PolyLR), "epoch" once
    after every epoch's batches, before validation.  Anything else is a ValueError.  None: nothing changes."""
    if scheduler_interval not in ("step", "epoch"):
        raise ValueError(f'train_model: scheduler_interval must be "step" or "epoch", got {scheduler_interval!r}')
    from .freeze import freeze as _freeze, unfreeze as _unfreeze
    from .losses import DistillLoss
    if isinstance(criterion, DistillLoss) and _is_rank0():
        print(f"Distils from a {type(criterion.teacher).__name__} (ce {criterion.ce:g}, kd {criterion.kd:g}, "
              f"temperature {criterion.temperature:g}, unlabelled pixels "
              f"{'distilled' if criterion.kd_ignored else 'left out'}); validation uses the hard-label loss")
    if freeze is not None:
        if isinstance(freeze, (str, nn.Module)):
            freeze = [freeze]
        freeze = list(freeze)
        _freeze(model, freeze)
        if _is_rank0():
            names = ", ".join(f if isinstance(f, str) else type(f).__name__ for f in freeze)
            until = "the whole run" if freeze_epochs is None else f"{freeze_epochs} epoch(s)"
            print(f"Frozen for {until}: {names} (parameters and BatchNorm statistics)")
    if ema is not None and _is_rank0():
        print(f"EMA of the weights (decay {ema.decay:g}{', warm-up' if ema.warmup else ''}): "
              + ("validation and best_checkpoint use the averaged weights" if val_loader is not None else
                 "no val_loader, so nothing is validated")
              + ("; the averaged weights are saved every epoch" if ema_checkpoint_pattern else ""))
    best_val_loss = float("inf")  # stays inf without a val_loader, as in the reference (src/train.py:46-76)
    for epoch in range(epochs):
        if freeze is not None and freeze_epochs is not None and epoch == freeze_epochs:
            _unfreeze(model, freeze)
            if _is_rank0():
                print(f"Unfrozen before epoch {epoch + 1}: {names}")
        sampler = getattr(train_loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)  # DistributedWeightedSampler: a new shared draw per epoch
        kw = {} if scheduler is None or scheduler_interval != "step" else {"scheduler": scheduler}
        avg_train_loss = train_one_epoch(model, train_loader, criterion, optimizer, device, epoch, epochs, progress,
                                         augment, max_grad_norm, ema, **kw)
        if scheduler is not None and scheduler_interval == "epoch":
            scheduler.step()
        val = None
        if val_loader is not None:  # every rank: validate() all-reduces
            with ema.applied() if ema is not None else contextlib.nullcontext():
                kw = {} if val_tta is None else {"tta": val_tta}  # None: the call as it always was
                val = validate(model, val_loader, criterion, device, progress, epoch, epochs, **kw)
        if _is_rank0():
            if val is not None:
                print(f"\nEpoch {epoch + 1}/{epochs}:")
            print(f"  Training Loss: {avg_train_loss:.4f}")
            if val is not None:
                print(f"  Validation Loss: {val['loss']:.4f}")
                if val["loss"] < best_val_loss:
                    print("  Validation loss improved! Saving model...")
                    if best_checkpoint:
                        os.makedirs(os.path.dirname(best_checkpoint) or ".", exist_ok=True)
                        torch.save(ema.averaged_state_dict() if ema is not None else
                                   getattr(model, "module", model).state_dict(), best_checkpoint)
            if checkpoint_pattern:
                path = checkpoint_pattern.format(epoch=epoch + 1)
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                core = getattr(model, "module", model)
                torch.save(core.state_dict(), path)
            if ema is not None and ema_checkpoint_pattern:
                path = ema_checkpoint_pattern.format(epoch=epoch + 1)
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                torch.save(ema.averaged_state_dict(), path)
        if val is not None and val["loss"] < best_val_loss:  # every rank returns the same dict
            best_val_loss = val["loss"]
    if _is_rank0():
        print(f"Training completed. Best validation loss: {best_val_loss:.4f}")
