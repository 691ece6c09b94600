"""The "poly" learning-rate schedule of the DeepLab / PSPNet / BiSeNet recipes, with a linear warm-up.

    opt = seg_amd.SGD(seg_amd.decay_groups(model, 5e-4), lr=1e-2, momentum=0.9, nesterov=True)
    sched = seg_amd.PolyLR(opt, total_iters=epochs * len(loader), warmup_iters=1000)
    seg_amd.train_model(model, loader, criterion, opt, device, epochs, scheduler=sched)

Per iteration t (scheduler.last_epoch; train_one_epoch calls step() after every optimizer step), per group:
    poly(t) = min_lr + (base_lr - min_lr) * (1 - min(t, T) / T) ** power
    lr(t)   = poly(t) * (warmup_ratio + (1 - warmup_ratio) * t / warmup_iters)    for t < warmup_iters
            = poly(t)                                                             otherwise
The warm-up factor reaches 1 at t = warmup_iters, so the two branches meet there.  Closed form: the value depends on
t alone, never on the group's current lr, so state_dict() / load_state_dict() resume from `last_epoch` and nothing
drifts.  torch.optim.lr_scheduler.PolynomialLR(total_iters=T, power=p) is the case without warm-up and min_lr.
"""
from __future__ import annotations

from torch.optim.lr_scheduler import LRScheduler


class PolyLR(LRScheduler):
    def __init__(self, optimizer, total_iters: int, power: float = 0.9, min_lr: float = 0.0, warmup_iters: int = 0,
                 warmup_ratio: float = 0.1, last_epoch: int = -1):
        if not total_iters >= 1:
            raise ValueError(f"PolyLR: total_iters must be >= 1, got {total_iters}")
        if not power > 0:
            raise ValueError(f"PolyLR: power must be positive, got {power}")
        if not 0 <= warmup_iters < total_iters:
            raise ValueError(f"PolyLR: warmup_iters must be in [0, total_iters), got {warmup_iters}")
        if not 0 < warmup_ratio <= 1:
            raise ValueError(f"PolyLR: warmup_ratio must be in (0, 1], got {warmup_ratio}")
        for group in optimizer.param_groups:
            base = group.get("initial_lr", group["lr"])
            if not 0 <= min_lr < base:
                raise ValueError(f"PolyLR: min_lr must be in [0, base lr = {base}), got {min_lr}")
        self.total_iters = total_iters
        self.power = power
        self.min_lr = min_lr
        self.warmup_iters = warmup_iters
        self.warmup_ratio = warmup_ratio
        super().__init__(optimizer, last_epoch)

    def _lr_at(self, base_lr: float, t: int) -> float:
        lr = self.min_lr + (base_lr - self.min_lr) * (1 - min(t, self.total_iters) / self.total_iters) ** self.power
        if t < self.warmup_iters:
            lr *= self.warmup_ratio + (1 - self.warmup_ratio) * t / self.warmup_iters
        return lr

    def get_lr(self):
        return [self._lr_at(base, self.last_epoch) for base in self.base_lrs]

    def _get_closed_form_lr(self):
        return self.get_lr()
