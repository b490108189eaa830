"""Fine-tuning helpers: frozen layers and eval-mode BatchNorm.

``freeze`` is the reference's ``freeze_layers`` (yolov8/tools/utils.py:84-94: a parameter is frozen
when any pattern is a substring of its name) plus what every detection fine-tuning recipe adds to it:
the BatchNorm modules of the frozen part go to eval mode (mmdet ``norm_eval=True``, torchvision
``FrozenBatchNorm2d``) and STAY there across ``model.train()``, which nn.Module.train would undo.

Nothing here is needed for the plan to do the right thing: it reads ``requires_grad`` and
``bn.training`` from the modules themselves (runner.train_state), so the reference's own
``freeze_layers`` and a hand-written ``m.bn.eval()`` get the same backward skip and running-statistics
routes.  What this module adds is the persistence of the eval-mode set.
"""
from __future__ import annotations

from torch import nn

_ATTR = "_yms_norm_eval"      # model.__dict__: the BN modules kept in eval mode (YOLOv8.train re-applies it)
_FROZEN = "_yms_frozen"       # model.__dict__: the parameters freeze() turned off (unfreeze turns only these on)
_BN = nn.modules.batchnorm._BatchNorm


def _keep_eval(model, bns):
    kept = model.__dict__.setdefault(_ATTR, [])
    for bn in bns:
        if not any(bn is k for k in kept):
            kept.append(bn)
        bn.eval()


def reapply(model):
    """Put the recorded BN modules back into eval mode (after an nn.Module.train(mode) walk)."""
    for bn in model.__dict__.get(_ATTR, ()):
        bn.eval()


def freeze(model, patterns, norm_eval=True):
    """Freeze every parameter whose name contains one of `patterns` -> the frozen names.
    norm_eval: every BatchNorm module whose parameters are now all frozen goes to eval mode (running
    statistics used and left unchanged) and stays there across model.train()."""
    patterns = list(patterns)
    frozen = []
    mine = model.__dict__.setdefault(_FROZEN, [])
    for name, p in model.named_parameters():
        if any(pat in name for pat in patterns):
            if p.requires_grad:
                mine.append(p)
            p.requires_grad = False
            frozen.append(name)
    if norm_eval:
        _keep_eval(model, [m for m in model.modules() if isinstance(m, _BN)
                           and all(not p.requires_grad for p in m.parameters(recurse=False))])
    return frozen


def norm_eval(model, patterns=None):
    """Put the BatchNorm modules whose name contains one of `patterns` (None: all of them) into eval
    mode, persistently; no parameter is frozen.  -> their names."""
    hit = [(n, m) for n, m in model.named_modules() if isinstance(m, _BN)
           and (patterns is None or any(pat in n for pat in patterns))]
    _keep_eval(model, [m for _, m in hit])
    return [n for n, _ in hit]


def unfreeze(model):
    """Undo freeze and norm_eval: the parameters freeze turned off require a gradient again (one that
    was frozen before, like the head's fixed DFL weight, stays so) and the recorded BN modules follow the
    model's mode."""
    for p in model.__dict__.pop(_FROZEN, ()):
        p.requires_grad = True
    for bn in model.__dict__.pop(_ATTR, ()):
        bn.train(model.training)
