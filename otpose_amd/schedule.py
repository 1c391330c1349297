"""Learning-rate schedules of the reference training loop (train.py:58-59, thirdparty/utils/train_utils.py:140-205,
thirdparty/utils/lr_schedulers.py): a linear warm-up from ``warmup_start_lr`` to each group's base rate, then cosine
annealing or a multi-step decay.  The reference steps its scheduler after EVERY ``optimizer.step()``
(script/Common.py:143-144), so every "epoch" argument below counts iterations.

The schedulers only read and write ``group["lr"]`` of a ``torch.optim.Optimizer`` - the plain torch optimizers and
:class:`otpose_amd.optim.FusedAdamW` / :class:`otpose_amd.optim.FusedSGD` alike; the fused ones read it at every step.
Saving a scheduler in a checkpoint is left out, as in the reference.
"""
from __future__ import annotations

import math
from bisect import bisect_right
from collections import Counter

import torch
from torch.optim.lr_scheduler import LRScheduler


class _LinearWarmup(LRScheduler):
    """Iterations ``0 .. warmup_epochs - 1`` climb linearly from ``warmup_start_lr`` and reach the base rate at iteration
    ``warmup_epochs - 1``; iteration ``warmup_epochs`` is set to the base rate exactly.  ``get_lr()`` is the chainable form
    (the next rate from the current one), ``_get_closed_form_lr()`` the rate as a function of ``last_epoch`` alone, which
    torch uses for ``step(epoch)``."""

    def __init__(self, optimizer, warmup_epochs, warmup_start_lr, last_epoch):
        self.warmup_epochs = warmup_epochs
        self.warmup_start_lr = warmup_start_lr
        super().__init__(optimizer, last_epoch)

    def _groups(self):
        return zip(self.base_lrs, self.optimizer.param_groups)

    def _warmup_chain(self):
        """The chainable rates up to and including iteration ``warmup_epochs``, or None behind it."""
        t = self.last_epoch
        if t == 0:
            return [self.warmup_start_lr] * len(self.base_lrs)
        if t < self.warmup_epochs:
            return [g["lr"] + (base - self.warmup_start_lr) / (self.warmup_epochs - 1) for base, g in self._groups()]
        if t == self.warmup_epochs:
            return list(self.base_lrs)
        return None

    def _warmup_closed(self):
        t = self.last_epoch
        if t < self.warmup_epochs:
            return [self.warmup_start_lr + t * (base - self.warmup_start_lr) / (self.warmup_epochs - 1)
                    for base in self.base_lrs]
        return None

    def get_lr(self):
        lrs = self._warmup_chain()
        return lrs if lrs is not None else self._after_warmup_chain()

    def _get_closed_form_lr(self):
        lrs = self._warmup_closed()
        return lrs if lrs is not None else self._after_warmup_closed()


class LinearWarmupCosineAnnealingLR(_LinearWarmup):
    """Linear warm-up, then half a cosine from the base rate down to ``eta_min`` at iteration ``max_epochs``; behind
    ``max_epochs`` the cosine goes on periodically (back up), as ``torch.optim.lr_scheduler.CosineAnnealingLR`` does."""

    def __init__(self, optimizer, warmup_epochs, max_epochs, warmup_start_lr=0.0, eta_min=1e-8, last_epoch=-1):
        self.max_epochs = max_epochs
        self.eta_min = eta_min
        super().__init__(optimizer, warmup_epochs, warmup_start_lr, last_epoch)

    def _after_warmup_chain(self):
        span = self.max_epochs - self.warmup_epochs
        t = self.last_epoch
        if (t - 1 - self.max_epochs) % (2 * span) == 0:
            # the bottom of a period: the quotient below would be 0 / 0, so the rate restarts by the first cosine increment
            return [g["lr"] + (base - self.eta_min) * (1 - math.cos(math.pi / span)) / 2 for base, g in self._groups()]
        now = 1 + math.cos(math.pi * (t - self.warmup_epochs) / span)
        before = 1 + math.cos(math.pi * (t - self.warmup_epochs - 1) / span)
        return [now / before * (g["lr"] - self.eta_min) + self.eta_min for g in self.optimizer.param_groups]

    def _after_warmup_closed(self):
        span = self.max_epochs - self.warmup_epochs
        c = 1 + math.cos(math.pi * (self.last_epoch - self.warmup_epochs) / span)
        return [self.eta_min + 0.5 * (base - self.eta_min) * c for base in self.base_lrs]


class LinearWarmupMultiStepLR(_LinearWarmup):
    """Linear warm-up, then the rate is multiplied by ``gamma`` whenever the iteration count behind the warm-up reaches a
    milestone (a milestone listed k times multiplies by ``gamma ** k``)."""

    def __init__(self, optimizer, warmup_epochs, milestones, warmup_start_lr=0.0, gamma=0.1, last_epoch=-1):
        self.milestones = Counter(milestones)
        self.gamma = gamma
        super().__init__(optimizer, warmup_epochs, warmup_start_lr, last_epoch)

    def _after_warmup_chain(self):
        hits = self.milestones.get(self.last_epoch - self.warmup_epochs, 0)
        if not hits:
            return [g["lr"] for g in self.optimizer.param_groups]
        return [g["lr"] * self.gamma ** hits for g in self.optimizer.param_groups]

    def _after_warmup_closed(self):
        passed = bisect_right(sorted(self.milestones.elements()), self.last_epoch - self.warmup_epochs)
        return [base * self.gamma ** passed for base in self.base_lrs]


def make_scheduler(optimizer, cfg, num_iters_per_epoch, last_epoch=-1):
    """The reference's ``make_scheduler`` (thirdparty/utils/train_utils.py:140-205); step the result once per iteration.

    ======================  =================================================  ==========================================
    ``TRAIN.LR_SCHEDULER``  ``TRAIN.WARMUP`` true                              ``TRAIN.WARMUP`` false
    ======================  =================================================  ==========================================
    ``CosineAnnealingLR``   :class:`LinearWarmupCosineAnnealingLR`,            ``torch...CosineAnnealingLR``,
                            ``WARMUP_EPOCHS * iters`` warm-up steps,           ``T_max = EPOCHS * iters``
                            ``(END_EPOCH + WARMUP_EPOCHS) * iters`` in all
    ``MultiStepLR``         :class:`LinearWarmupMultiStepLR`, ``GAMMA``        ``torch...MultiStepLR``, ``GAMMA``
    ======================  =================================================  ==========================================

    The reference builds the milestones of both ``MultiStepLR`` branches from an empty list (train_utils.py:169, :195), not
    from ``TRAIN.MILESTONES``: the rate stays constant behind the warm-up and ``GAMMA`` is never applied.  That is
    reproduced here on purpose.  Any other name raises ``TypeError("Unsupported scheduler!")``.  ``last_epoch`` goes to
    torch unchanged (anything but -1 needs ``initial_lr`` in the groups, as torch says)."""
    name = cfg.TRAIN.LR_SCHEDULER
    if name not in ("CosineAnnealingLR", "MultiStepLR"):
        raise TypeError("Unsupported scheduler!")
    milestones = []                                    # the reference's (empty) list: see the docstring
    if cfg.TRAIN.WARMUP:
        warmup_steps = cfg.TRAIN.WARMUP_EPOCHS * num_iters_per_epoch
        max_steps = (cfg.TRAIN.END_EPOCH + cfg.TRAIN.WARMUP_EPOCHS) * num_iters_per_epoch
        if name == "CosineAnnealingLR":
            return LinearWarmupCosineAnnealingLR(optimizer, warmup_steps, max_steps, last_epoch=last_epoch)
        return LinearWarmupMultiStepLR(optimizer, warmup_steps, milestones, gamma=cfg.TRAIN.GAMMA, last_epoch=last_epoch)
    if name == "CosineAnnealingLR":
        return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, cfg.TRAIN.EPOCHS * num_iters_per_epoch,
                                                          last_epoch=last_epoch)
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma=cfg.TRAIN.GAMMA, last_epoch=last_epoch)
