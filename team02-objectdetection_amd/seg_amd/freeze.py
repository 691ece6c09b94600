"""Fine-tuning: freeze parts of a segamd model -- no gradients for their parameters, and their BatchNorm
layers left on their running statistics.

    seg_amd.freeze(model)                        # the pretrained backbone: parameters and BatchNorm statistics
    seg_amd.train_model(model, ...)              # trains the decoder; model.train() keeps the freeze
    seg_amd.unfreeze(model)                      # then everything

`freeze` sets `requires_grad_(False)` on the parameters of the named submodules (params=True) and puts their
`BatchNorm2d` layers in eval mode (bn_stats=True); the model's `train()` puts those layers back in eval after every
mode change, so `train_one_epoch`, `validate` and a caller's own `model.train()` keep them there.  The HIP engine
reads both per layer (seg_amd/engine.py: a frozen BatchNorm runs on its running statistics and leaves them alone;
the backward stops at the gradient frontier), and so does the CPU composition, which runs the modules themselves.

The bookkeeping is a plain dict in `model.__dict__` (submodule name -> what was frozen): no state_dict key, no
registered submodule.  A parameter without a gradient has `.grad is None`, which `torch.optim.Adam` and
`seg_amd.Adam` skip; the Adam state of a parameter unfrozen later starts at step 0, as in torch.
"""
from __future__ import annotations

from torch import nn

_ATTR = "_segamd_frozen"


def _core(model):
    return getattr(model, "module", model)  # a DataParallel wrapper's model


def _names(model, what):
    """Submodule names of `model` for a name, a module, or an iterable of either."""
    if isinstance(what, (str, nn.Module)):
        what = [what]
    by_id = None
    out = []
    for w in what:
        if isinstance(w, str):
            model.get_submodule(w)  # AttributeError for an unknown name
            name = w
        elif isinstance(w, nn.Module):
            if by_id is None:
                by_id = {}
                for n, m in model.named_modules():
                    by_id.setdefault(id(m), n)
            if id(w) not in by_id:
                raise ValueError(f"{type(w).__name__} is not a submodule of {type(model).__name__}")
            name = by_id[id(w)]
        else:
            raise TypeError(f"freeze: expected a submodule name or a module, got {type(w).__name__}")
        if name not in out:
            out.append(name)
    return out


def _batchnorms(model, name):
    return [m for m in model.get_submodule(name).modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]


def keep_frozen(model) -> None:
    """Put the BatchNorm layers frozen with bn_stats=True back in eval mode (after a train() / eval() call)."""
    for name, f in model.__dict__.get(_ATTR, {}).items():
        if f["bn_stats"]:
            for bn in _batchnorms(model, name):
                bn.training = False


def freeze(model, what="backbone", *, params: bool = True, bn_stats: bool = True):
    """Freeze the submodules `what` of `model` (a name such as "backbone", "down1", "inc"; a module; or an iterable
    of either): params -- their parameters get no gradient; bn_stats -- their BatchNorm layers run on, and keep, their
    running statistics, whatever mode the model is put in.  Returns the model."""
    model = _core(model)
    book = model.__dict__.setdefault(_ATTR, {})
    for name in _names(model, what):
        f = book.setdefault(name, {"params": False, "bn_stats": False})
        f["params"], f["bn_stats"] = f["params"] or params, f["bn_stats"] or bn_stats
        if params:
            model.get_submodule(name).requires_grad_(False)
    keep_frozen(model)
    return model


def unfreeze(model, what=None):
    """Undo freeze() for the submodules `what` (None: everything frozen): their parameters require gradients again
    and their BatchNorm layers follow the model's mode.  What another, still frozen entry covers stays frozen."""
    model = _core(model)
    book = model.__dict__.get(_ATTR, {})
    for name in (list(book) if what is None else _names(model, what)):
        f = book.pop(name, None)
        if f is None:
            continue
        if f["params"]:
            model.get_submodule(name).requires_grad_(True)
        if f["bn_stats"]:
            for bn in _batchnorms(model, name):
                bn.training = model.training
    for name, f in book.items():  # overlapping entries that remain
        if f["params"]:
            model.get_submodule(name).requires_grad_(False)
    keep_frozen(model)
    return model


def frozen_modules(model) -> dict:
    """What is frozen now: {submodule name: {"params": bool, "bn_stats": bool}}, in the order it was frozen."""
    return {n: dict(f) for n, f in _core(model).__dict__.get(_ATTR, {}).items()}
