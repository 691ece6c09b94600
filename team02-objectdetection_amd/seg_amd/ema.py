"""Exponential moving average of a model's weights, kept by one HIP launch per step (csrc/adam.hip).

`EMA(model, decay)` is what timm's `ModelEmaV2`, `AveragedModel(..., get_ema_multi_avg_fn(decay))` and mmseg's EMA
hook keep: after every optimizer step `e = e + (1 - decay) * (p - e)` over every floating-point `state_dict` entry --
parameters and BatchNorm running statistics.  The averaged model is the one to evaluate, checkpoint and deploy.

The average lives in shadow tensors, not in a second model.  `update()` is one seg_ema_update launch over a chunk map
of the optimizer's kind; `applied()` / `swap()` exchange the shadows' values with the live tensors' in place
(seg_ema_swap), so inside `applied()` the model itself holds the averaged weights.  No pointer changes: the model's
recorded plans, `forward_metrics`, `validate` and `Predictor.refresh()` run on them as they are, with no second set
of plans or buffers.  What the engine derives from the weights (packed and bf16 weights, eval BatchNorm coefficients)
is formed anew by every forward's own launches, so a swap needs no refresh; a `Predictor` keeps its folded weights
until `refresh()`, so the recipe there is `with ema.applied(): predictor.refresh()`.

CUDA models go through libsegamd only (contiguous fp32 tensors; anything else raises, a missing library raises);
CPU models (the torch-op composition) run the same class on `torch._foreach_lerp_` and torch copies.
"""
from __future__ import annotations

import contextlib

import torch

from ._lib import call
from .optim import _CHUNK, _chunk_map


def warmup_decay(decay: float, n: int) -> float:
    """The decay of update number n (0-based) with warm-up: min(decay, (1 + n) / (10 + n))."""
    return min(decay, (1 + n) / (10 + n))


class EMA:
    def __init__(self, model, decay: float = 0.999, warmup: bool = False):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"EMA decay must be in [0, 1], got {decay}")
        self.model = getattr(model, "module", model)  # DataParallel: the wrapped module's own keys
        self.decay, self.warmup = decay, bool(warmup)
        self.num_updates = 0
        self._last = 0          # what the last update() added to num_updates (undo_update_count)
        self._swapped = False   # the model holds the averaged values, the shadows the live ones
        self._applied = False
        # where each floating-point state_dict entry lives: (the owning module's _parameters / _buffers dict, name).
        # Read again at every use: load_state_dict(assign=True), p.data = ... and DataParallel's flat BatchNorm
        # buffers replace the tensor (or its storage), never the dict.
        # A module registered under two names (MobileNetV2UNet's encoder stages alias backbone.features) gives two
        # state_dict keys for one tensor: they share one shadow, so no element is averaged or exchanged twice.
        where = {}
        for prefix, mod in self.model.named_modules(remove_duplicate=False):
            dot = prefix + "." if prefix else ""
            for n in mod._parameters:
                where[dot + n] = (mod._parameters, n)
            for n in mod._buffers:
                where[dot + n] = (mod._buffers, n)
        self.names, self._slot, self._where = [], {}, []  # every float key; key -> shadow index; one per tensor
        seen = {}
        for k, v in self.model.state_dict().items():
            if v.is_floating_point():
                if k not in where:
                    raise NotImplementedError(f"EMA: state_dict entry {k!r} is not a parameter or buffer of a submodule")
                d, n = where[k]
                i = seen.get(id(d[n]))
                if i is None:
                    i = seen[id(d[n])] = len(self._where)
                    self._where.append((d, n))
                self.names.append(k)
                self._slot[k] = i
        self._first = {i: k for k, i in reversed(list(self._slot.items()))}  # a name per shadow, for messages
        srcs = self._sources()
        self._check(srcs)
        with torch.no_grad():
            self.shadows = [s.detach().clone() for s in srcs]
        self._key = self._table = self._chunks = None
        if srcs and srcs[0].is_cuda:
            self._bind(srcs)

    # ---------------------------------------------------------------- sources and the device table
    def _sources(self):
        return [d[n] for d, n in self._where]

    def _check(self, srcs):
        if not srcs or not srcs[0].is_cuda:
            return
        dev = srcs[0].device
        for i, s in enumerate(srcs):
            k = self._first[i]
            if not (s.is_cuda and s.device == dev and s.dtype == torch.float32 and s.is_contiguous()):
                raise NotImplementedError(f"seg_amd.EMA needs contiguous fp32 tensors on one CUDA device ({k}: "
                                          f"{s.dtype}, {s.device}, contiguous={s.is_contiguous()})")

    def _follow(self, srcs):
        """Shadows follow their sources to another device (model.to()); their values are kept."""
        for i, s in enumerate(srcs):
            k, e = self._first[i], self.shadows[i]
            if e.shape != s.shape:
                raise RuntimeError(f"EMA: {k} changed shape from {tuple(e.shape)} to {tuple(s.shape)}")
            if e.device != s.device or e.dtype != s.dtype:
                self.shadows[i] = e.to(device=s.device, dtype=s.dtype)

    def _bind(self, srcs):
        """The SegEmaTensor table and the chunk map on the device, rebuilt only when a source's storage moved."""
        key = tuple(s.data_ptr() for s in srcs)
        if key == self._key:
            return
        self._check(srcs)
        self._follow(srcs)
        dev = srcs[0].device
        rows = [(e.data_ptr(), s.data_ptr(), s.numel()) for e, s in zip(self.shadows, srcs)]
        self._table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(dev)
        self._chunks = _chunk_map([s.numel() for s in srcs], dev)
        self._key = key

    def _busy(self) -> bool:
        return any(p.busy for p in self.model.__dict__.get("_segamd_plans", {}).values())

    # ---------------------------------------------------------------- the average
    def current_decay(self) -> float:
        """The decay the next update() uses."""
        return warmup_decay(self.decay, self.num_updates) if self.warmup else self.decay

    @torch.no_grad()
    def update(self, skip_if_nonzero: torch.Tensor | None = None):
        """e += (1 - decay) * (p - e) over every shadow: one seg_ema_update launch on torch's current stream.
        skip_if_nonzero: the optimizer step's flag tensor (seg_amd.Adam.step) -- when it holds a non-zero value as the
        kernel runs, nothing is averaged.  num_updates advances at queue time; undo_update_count() takes it back."""
        if self._swapped:
            raise RuntimeError("EMA.update() while the averaged weights are swapped into the model")
        w = 1.0 - self.current_decay()  # in double; rounded to fp32 once, at the call
        self.num_updates += 1
        self._last = 1
        srcs = self._sources()
        if not srcs:
            return
        if not srcs[0].is_cuda:
            if skip_if_nonzero is not None and float(skip_if_nonzero.reshape(-1)[0]) != 0:
                return
            self._follow(srcs)
            torch._foreach_lerp_(self.shadows, [s.detach() for s in srcs], w)
            return
        if skip_if_nonzero is not None and not (skip_if_nonzero.is_cuda and skip_if_nonzero.dtype == torch.float32
                                                and skip_if_nonzero.numel() >= 1):
            raise ValueError("skip_if_nonzero must be a float32 CUDA tensor")
        self._bind(srcs)
        call("seg_ema_update", self._table.data_ptr(), self._chunks.data_ptr(), self._chunks.shape[0], _CHUNK, w,
             skip_if_nonzero.data_ptr() if skip_if_nonzero is not None else None,
             torch.cuda.current_stream(srcs[0].device).cuda_stream)

    def undo_update_count(self):
        """Take back the num_updates advance of the last update() -- for one the device skipped (skip_if_nonzero):
        the warm-up schedule then continues where it was, as Adam.undo_step_count() does for the step counters."""
        self.num_updates -= self._last
        self._last = 0

    # ---------------------------------------------------------------- exchange in place
    @torch.no_grad()
    def swap(self):
        """Exchange the shadows' values with the live tensors' in place (one seg_ema_swap launch).  Raises, and
        swaps nothing, while a recorded plan of the model is between its forward and its backward: that backward
        reads the weights the forward ran on."""
        if self._busy():
            raise RuntimeError("EMA.swap(): a forward of the model is still waiting for its backward")
        srcs = self._sources()
        if srcs and srcs[0].is_cuda:
            self._bind(srcs)
            call("seg_ema_swap", self._table.data_ptr(), self._chunks.data_ptr(), self._chunks.shape[0], _CHUNK,
                 torch.cuda.current_stream(srcs[0].device).cuda_stream)
        elif srcs:
            self._follow(srcs)
            live = [s.detach() for s in srcs]
            tmp = [s.clone() for s in live]
            torch._foreach_copy_(live, self.shadows)
            torch._foreach_copy_(self.shadows, tmp)
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def applied(self):
        """Inside, the model holds the averaged weights and statistics (and the shadows the live ones); on exit
        both are back, bit for bit.  Nesting raises."""
        if self._applied or self._swapped:
            raise RuntimeError("EMA.applied(): the averaged weights are already swapped in")
        self.swap()
        self._applied = True
        try:
            yield self
        finally:
            self._applied = False
            self.swap()

    # ---------------------------------------------------------------- the averaged model as values
    @torch.no_grad()
    def averaged_state_dict(self) -> dict:
        """The model's state_dict with the averaged values (clones); integer buffers (num_batches_tracked) are the
        live model's.  Same keys, same order: loads with strict=True wherever the model's own does."""
        sd = self.model.state_dict()
        if self._swapped:  # the model holds them right now
            return type(sd)((k, v.detach().clone()) for k, v in sd.items())
        avg = {k: self.shadows[self._slot[k]] for k in self.names}
        return type(sd)((k, (avg[k] if k in avg else v).detach().clone()) for k, v in sd.items())

    @torch.no_grad()
    def copy_to(self, other_model):
        """Write the averaged values (and the live integer buffers) into another model of the same architecture."""
        other = getattr(other_model, "module", other_model)
        dst = other.state_dict()
        src = self.averaged_state_dict()
        if dst.keys() != src.keys():
            raise KeyError(f"EMA.copy_to: state_dict keys differ: {sorted(set(dst) ^ set(src))[:5]}")
        for k, v in dst.items():
            v.copy_(src[k])
        return other_model

    # ---------------------------------------------------------------- resuming
    def state_dict(self) -> dict:
        if self._swapped:
            raise RuntimeError("EMA.state_dict() while the averaged weights are swapped into the model")
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates,
                "shadow": {k: self.shadows[self._slot[k]].detach().clone() for k in self.names}}

    @torch.no_grad()
    def load_state_dict(self, state: dict):
        if self._swapped:
            raise RuntimeError("EMA.load_state_dict() while the averaged weights are swapped into the model")
        shadow = state["shadow"]
        if set(shadow) != set(self.names):
            raise KeyError(f"EMA.load_state_dict: shadow names differ: {sorted(set(shadow) ^ set(self.names))[:5]}")
        decay = float(state["decay"])
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"EMA decay must be in [0, 1], got {decay}")
        for k in self.names:
            self.shadows[self._slot[k]].copy_(shadow[k])  # in place: the device table stays valid
        self.decay, self.warmup, self.num_updates = decay, bool(state["warmup"]), int(state["num_updates"])
        self._last = 0
