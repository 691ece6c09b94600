"""Adam, AdamW and SGD with a one-launch HIP step, and global-norm gradient clipping (csrc/adam.hip).

`Adam` is the drop-in for the reference's `optim.Adam(model.parameters(), lr=1.5e-4)` (main.py:100),
stepped once per batch by train_model (src/train.py:39): same constructor, same
param_groups and state_dict layout (state 'step' as a CPU tensor, 'exp_avg',
'exp_avg_sq'), so checkpoints move between the two.  torch's foreach Adam issues ~8
multi-tensor launches per step, each streaming the 6.5 M parameters' p / g / m / v
again; seg_adam_step reads and writes each element once with the same fp32 operation
order (see adam.hip).  Supported: the reference's configuration (no weight decay, no
amsgrad, not maximize) on CUDA fp32 dense tensors; anything else raises -- there is no
silent fallback.

`AdamW` is the same for `torch.optim.AdamW` (decoupled weight decay): one seg_adamw_step launch per
parameter group, torch's `_multi_tensor_adam` arithmetic with `p *= 1 - lr * weight_decay` in front; per-group
lr / betas / eps / weight_decay, lr read at every step (torch.optim.lr_scheduler.* work unchanged).  Weight decay
stays refused by `Adam` (its L2 form, added to the gradient, is not implemented), as do amsgrad, maximize,
capturable and differentiable by both.

`SGD` is the same for `torch.optim.SGD`, the optimizer of the DeepLab / PSPNet / BiSeNet recipes (momentum 0.9,
often Nesterov, L2 weight decay on the weights, a poly schedule: seg_amd/schedule.py): one seg_sgd_step launch per
group reads p, g and the momentum buffer and writes p and the buffer, where torch's foreach SGD makes up to five
multi-tensor passes and a temporary copy of the gradients.  torch's `_multi_tensor_sgd` arithmetic in its order,
its first step included (the buffer starts as a copy of g + weight_decay * p, without dampening); param_groups and
state ('momentum_buffer' alone) are torch's.  Refused: maximize, differentiable.

Clipping: `grad_norm` (the global L2 norm, the clip coefficient and a non-finite flag, on the device, no host
wait), `clip_grad_norm_` (torch.nn.utils.clip_grad_norm_'s contract, L2 only) and `step(grad_scale=...)`, which
multiplies each gradient element by a device float as the step loads it -- `.grad` is never rewritten.
`decay_groups` builds the usual two parameter groups (weights decayed, biases and BatchNorm not).
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from ._lib import call, query

_CHUNK = 4096  # elements per block
_CHUNK_MAPS = {}  # (sizes, device) -> chunk map, for the functions that have no optimizer to keep it


def _chunk_map(sizes, device):
    """Device int64 [(tensor index, first element)] pairs covering every tensor in pieces of <= _CHUNK elements."""
    pairs = [(ti, s) for ti, n in enumerate(sizes) for s in range(0, n, _CHUNK)]
    return torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2).to(device)


class _OneLaunch:
    """What the one-launch optimizers share: the chunk-map cache, the checks of step()'s device arguments and of a
    parameter and its gradient, the closure, and the upload of the tensor table."""

    def _init_one_launch(self):
        self._chunk_maps = {}

    def _chunks(self, sizes, device):
        key = (tuple(sizes), device)
        cm = self._chunk_maps.get(key)
        if cm is None:
            cm = self._chunk_maps[key] = _chunk_map(sizes, device)
        return cm

    @staticmethod
    def _begin_step(closure, skip_if_nonzero, grad_scale):
        """Check step()'s two device arguments, then run the closure; returns its loss (None without one)."""
        for what, t in (("skip_if_nonzero", skip_if_nonzero), ("grad_scale", grad_scale)):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.numel() >= 1):
                raise ValueError(f"{what} must be a float32 CUDA tensor")
        if closure is None:
            return None
        with torch.enable_grad():
            return closure()

    def _check_tensors(self, ps):
        """The kernels index p and p.grad flatly through raw pointers: anything but dense contiguous fp32 CUDA
        tensors is refused, before any state is created for the group."""
        for p in ps:
            g = p.grad
            if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and not g.is_sparse
                    and p.is_contiguous() and g.is_contiguous()):
                raise NotImplementedError(
                    f"seg_amd.{type(self).__name__} needs contiguous fp32 CUDA parameters and gradients")

    @staticmethod
    def _upload(table, device):
        """The packed tensor table on `device`: through pinned memory, so that the copy does not wait for the GPU."""
        return table.pin_memory().to(device, non_blocking=True)


class _OneLaunchStep(_OneLaunch):
    """The host side of Adam and AdamW: argument checks, state, CPU step counters, the tensor table and the launch.
    _DECOUPLED: the class applies weight decay (AdamW's form); otherwise any weight decay is refused."""
    _DECOUPLED = False

    def _init_one_launch(self):
        super()._init_one_launch()
        self._last_steps = []  # the CPU step counters the last step() advanced (undo_step_count)

    @torch.no_grad()
    def step(self, closure=None, *, skip_if_nonzero: torch.Tensor | None = None,
             grad_scale: torch.Tensor | None = None):
        """One step.  skip_if_nonzero: a one-element fp32 device tensor; when it holds a non-zero value at the
        time the step runs on the GPU (stream order), the kernel leaves every parameter and moment unchanged --
        train_one_epoch passes the batch's out-of-range label count here so the step can be queued without a host
        wait; the CPU step counters advance at queue time, and the loop calls undo_step_count() before it raises, so
        a skipped step leaves 'step' where the reference's (which never reaches optimizer.step()) leaves it.
        grad_scale: a one-element fp32 device tensor (grad_norm(...)[1:2]); every gradient element is multiplied by
        it as it is loaded, bit for bit as if the gradients had been scaled in place first; .grad is not written."""
        name = type(self).__name__
        loss = self._begin_step(closure, skip_if_nonzero, grad_scale)
        self._last_steps = []
        wide = self._DECOUPLED or grad_scale is not None  # seg_adamw_step; else seg_adam_step_skip, as ever
        for group in self.param_groups:
            if group["amsgrad"] or group["maximize"] or group.get("capturable") or group.get("differentiable") \
                    or (not self._DECOUPLED and (group["weight_decay"] != 0 or group.get("decoupled_weight_decay"))):
                raise NotImplementedError(
                    f"seg_amd.{name} supports " + ("decoupled weight decay" if self._DECOUPLED else
                                                   "the reference's configuration (weight_decay=0)")
                    + " with amsgrad/maximize/capturable/differentiable off only")
            b1, b2 = group["betas"]
            lr, eps = float(group["lr"]), group["eps"]
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            self._check_tensors(ps)
            for p in ps:
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            sts = [self.state[p] for p in ps]
            steps = [st["step"] for st in sts]
            torch._foreach_add_(steps, 1)  # CPU step counters, as torch's foreach Adam keeps them
            self._last_steps += steps
            rows = []
            for p, st, t in zip(ps, sts, torch.stack(steps).tolist()):
                bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
                rows.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             p.numel(), -(lr / bc1), bc2 ** 0.5))
            if wide:  # + (decay, pad)
                tail = (1 - lr * group["weight_decay"] if self._DECOUPLED else 1.0, 0.0)
                rows = [r + tail for r in rows]
            device = ps[0].device
            table = self._upload(_pack_w(rows) if wide else _pack(rows), device)
            chunks = self._chunks([p.numel() for p in ps], device)
            skip = skip_if_nonzero.data_ptr() if skip_if_nonzero is not None else None
            stream = torch.cuda.current_stream(device).cuda_stream
            if wide:
                call("seg_adamw_step", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], _CHUNK, 1 - b1, b2,
                     1 - b2, eps, skip, grad_scale.data_ptr() if grad_scale is not None else None, stream)
            else:
                call("seg_adam_step_skip", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], _CHUNK, 1 - b1, b2,
                     1 - b2, eps, skip, stream)
        return loss

    def undo_step_count(self):
        """Take back the step-counter advance of the last step() -- for a step the device skipped
        (skip_if_nonzero): the bias corrections of the next real step are then the reference's.  The
        moments need nothing: a skipped step leaves them as they were (zeros for a new parameter, as torch's Adam
        would create them on its first step)."""
        if self._last_steps:
            torch._foreach_sub_(self._last_steps, 1)
        self._last_steps = []


class Adam(_OneLaunchStep, torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        self._init_one_launch()


class AdamW(_OneLaunchStep, torch.optim.AdamW):
    """torch.optim.AdamW with one seg_adamw_step launch per parameter group (module docstring)."""
    _DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        self._init_one_launch()


class SGD(_OneLaunch, torch.optim.SGD):
    """torch.optim.SGD (momentum, dampening, Nesterov, L2 weight decay) with one seg_sgd_step launch per parameter
    group (module docstring).  The state is torch's: 'momentum_buffer' alone, and only from the first step that had
    a gradient for the parameter; a buffer that load_state_dict brought continues its recurrence."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **kw):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, **kw)
        self._init_one_launch()

    def _init_one_launch(self):
        super()._init_one_launch()
        self._last_seeded = []  # the parameters whose momentum_buffer the last step() created (undo_step_count)

    @torch.no_grad()
    def step(self, closure=None, *, skip_if_nonzero: torch.Tensor | None = None,
             grad_scale: torch.Tensor | None = None):
        """One step; skip_if_nonzero and grad_scale as in Adam.step().  A parameter without a momentum_buffer gets
        one here (zeros at queue time) and the kernel seeds it with d = g + weight_decay * p, torch's first step;
        undo_step_count() removes the buffers of a step the device skipped.  Every group is checked before the first
        buffer is created and the first launch queued: a refused step changes nothing."""
        loss = self._begin_step(closure, skip_if_nonzero, grad_scale)
        self._last_seeded = []
        work = []
        for group in self.param_groups:
            if group["maximize"] or group.get("differentiable"):
                raise NotImplementedError("seg_amd.SGD supports maximize and differentiable off only")
            # the kernel is chosen on the fp32 value (seg_sgd_step's argument): a momentum that underflows there is
            # no momentum here either, so no buffer is created that no kernel would write
            momentum = ctypes.c_float(group["momentum"]).value
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            self._check_tensors(ps)
            bufs = None
            if momentum != 0:  # the buffers that exist (state is a defaultdict: get() creates no entry)
                bufs = []
                for p in ps:
                    st = self.state.get(p)
                    buf = st.get("momentum_buffer") if st else None
                    if buf is not None and not (buf.device == p.device and buf.dtype == torch.float32
                                                and not buf.is_sparse and buf.is_contiguous()
                                                and buf.shape == p.shape):
                        raise NotImplementedError("seg_amd.SGD needs contiguous fp32 CUDA momentum buffers")
                    bufs.append(buf)
            work.append((group, momentum, ps, bufs))
        for group, momentum, ps, bufs in work:
            if bufs is None:
                rows = [(p.data_ptr(), p.grad.data_ptr(), 0, 0, p.numel(), 0.0, 1.0, 1.0, 0.0) for p in ps]
            else:
                rows = []
                for p, buf in zip(ps, bufs):
                    seed = 0.0
                    if buf is None:
                        buf = torch.zeros_like(p, memory_format=torch.preserve_format)
                        self.state[p]["momentum_buffer"] = buf
                        self._last_seeded.append(p)
                        seed = 1.0
                    rows.append((p.data_ptr(), p.grad.data_ptr(), buf.data_ptr(), 0, p.numel(), 0.0, 1.0, 1.0, seed))
            device = ps[0].device
            table = self._upload(_pack_w(rows), device)
            chunks = self._chunks([p.numel() for p in ps], device)
            call("seg_sgd_step", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], _CHUNK, float(group["lr"]),
                 momentum, 1 - group["dampening"], float(group["weight_decay"]), int(bool(group["nesterov"])),
                 skip_if_nonzero.data_ptr() if skip_if_nonzero is not None else None,
                 grad_scale.data_ptr() if grad_scale is not None else None,
                 torch.cuda.current_stream(device).cuda_stream)
        return loss

    def undo_step_count(self):
        """Take back what the last step() changed on the host -- for a step the device skipped (skip_if_nonzero).
        SGD keeps no step counter; what a skipped step leaves behind is the momentum_buffer entries it created, still
        zero.  They go, so that state_dict() is what it was and the next real step seeds them as torch's first step
        does (buf = d, without dampening)."""
        for p in self._last_seeded:
            st = self.state.get(p)
            if st is not None:
                st.pop("momentum_buffer", None)
                if not st:
                    del self.state[p]
        self._last_seeded = []


def _pack(rows):
    """SegAdamTensor[] (include/segamd.h) as int64 words: 4 pointers, n, (step_size, bc2_sqrt)."""
    f = torch.tensor([[r[5], r[6]] for r in rows], dtype=torch.float32)
    words = torch.tensor([r[:5] for r in rows], dtype=torch.int64)
    return torch.cat([words, f.view(torch.int64)], dim=1).contiguous()


def _pack_w(rows):
    """SegAdamWTensor[] (include/segamd.h) as int64 words: 4 pointers, n, (step_size, bc2_sqrt), (decay, pad)."""
    f = torch.tensor([r[5:9] for r in rows], dtype=torch.float32)
    words = torch.tensor([r[:5] for r in rows], dtype=torch.int64)
    return torch.cat([words, f.view(torch.int64)], dim=1).contiguous()


# ------------------------------------------------------------------ gradient norm and clipping

def _with_grads(parameters):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    return [p for p in parameters if p.grad is not None]


def _grad_table(ps):
    """(table, chunk map) of the gradients of `ps` for seg_grad_sumsq / seg_grad_scale (only g and n are read)."""
    device = ps[0].grad.device
    for p in ps:
        g = p.grad
        if not (g.is_cuda and g.device == device and g.dtype == torch.float32 and not g.is_sparse
                and g.is_contiguous()):
            raise NotImplementedError("seg_amd.grad_norm needs contiguous fp32 gradients on one CUDA device")
    sizes = tuple(p.grad.numel() for p in ps)
    cm = _CHUNK_MAPS.get((sizes, device))
    if cm is None:
        if len(_CHUNK_MAPS) >= 8:
            _CHUNK_MAPS.clear()
        cm = _CHUNK_MAPS[(sizes, device)] = _chunk_map(sizes, device)
    rows = [(0, p.grad.data_ptr(), 0, 0, n, 0.0, 1.0, 1.0, 0.0) for p, n in zip(ps, sizes)]
    return _pack_w(rows).pin_memory().to(device, non_blocking=True), cm


def _norm(ps, max_norm):
    device = ps[0].grad.device
    table, cm = _grad_table(ps)
    out = torch.empty(3, dtype=torch.float32, device=device)
    if cm.shape[0] == 0:  # only empty gradients
        out.copy_(torch.tensor([0.0, 1.0, 0.0]))
        return out, table, cm
    work = torch.empty(query("seg_grad_norm_workspace_floats", cm.shape[0]), dtype=torch.float32, device=device)
    call("seg_grad_sumsq", table.data_ptr(), cm.data_ptr(), cm.shape[0], _CHUNK,
         0.0 if max_norm is None else float(max_norm), work.data_ptr(), out.data_ptr(),
         torch.cuda.current_stream(device).cuda_stream)
    return out, table, cm


def grad_norm(parameters, max_norm=None) -> torch.Tensor:
    """[norm, coef, nonfinite] as a 3-element fp32 device tensor, with no host wait: the global L2 norm of the
    gradients of `parameters` (those with `.grad is None` are skipped), the clip coefficient
    min(max_norm / (norm + 1e-6), 1) (1 without a max_norm; NaN for a NaN norm, as torch's clamp gives) and 1.0
    if the norm is inf or NaN.  Run to run the result is bitwise the same (fixed summation order, no atomics).
    `out[1:2]` is what `step(grad_scale=...)` takes.  No gradients at all: [0, 1, 0].  CUDA gradients only."""
    params = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    ps = _with_grads(params)
    if not ps:
        return torch.tensor([0.0, 1.0, 0.0], device=params[0].device if params else None)
    return _norm(ps, max_norm)[0]


def clip_grad_norm_(parameters, max_norm, error_if_nonfinite=False) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ for the L2 norm: scales the gradients in place so that their global norm is
    at most `max_norm` (> 0) and returns the norm before clipping as a 0-dim device tensor.  grad_norm followed by
    seg_grad_scale: two reads of the gradients and, only when something is clipped, one write; no host wait unless
    error_if_nonfinite, which reads the flag and raises RuntimeError as torch does.  CPU gradients (the CPU model
    composition) and an empty set go to torch's function."""
    if not float(max_norm) > 0:
        raise ValueError(f"clip_grad_norm_: max_norm must be positive, got {max_norm}")
    params = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    ps = _with_grads(params)
    if not ps or not ps[0].grad.is_cuda:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=error_if_nonfinite)
    out, table, cm = _norm(ps, max_norm)
    if error_if_nonfinite and float(out[2]):
        raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it "
                           "cannot be clipped. To disable this error and scale the gradients by the non-finite "
                           "norm anyway, set `error_if_nonfinite=False`")
    call("seg_grad_scale", table.data_ptr(), cm.data_ptr(), cm.shape[0], _CHUNK, out[1:2].data_ptr(),
         torch.cuda.current_stream(out.device).cuda_stream)
    return out[0]


def decay_groups(model, weight_decay: float):
    """Two parameter groups for AdamW: the weights of convolutions and linear layers (ndim > 1) with
    `weight_decay`; every bias and every BatchNorm weight and bias (and anything else) with 0.0.  Each parameter
    that requires a gradient appears exactly once; what seg_amd.freeze froze is left out."""
    decay, rest, seen = [], [], set()
    for mod in getattr(model, "module", model).modules():
        for name, p in mod.named_parameters(recurse=False):
            if id(p) in seen or not p.requires_grad:
                continue
            seen.add(id(p))
            is_weight = isinstance(mod, (nn.modules.conv._ConvNd, nn.Linear)) and name == "weight" and p.ndim > 1
            (decay if is_weight else rest).append(p)
    return [{"params": decay, "weight_decay": weight_decay}, {"params": rest, "weight_decay": 0.0}]
