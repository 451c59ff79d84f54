"""Learning-rate schedules for `Engine.set_lr` (pure Python, no device).

Each function maps the Adam step number t -- the 1-based index of the update about to run, the
same t as in Adam's bias corrections -- to a learning rate.  The trainers' `lr_schedule` argument
takes any callable of that form; bind the other arguments with functools.partial or a lambda:

    TRANSFORMER(cfg, ..., lr_schedule=lambda t: warmup_inverse_sqrt(t, 5e-4, 4000), grad_clip=1.0)
"""
from __future__ import annotations

import math


def constant(step: int, base_lr: float) -> float:
    return float(base_lr)


def warmup_inverse_sqrt(step: int, base_lr: float, warmup_steps: int) -> float:
    """Linear from 0 to base_lr over warmup_steps, then base_lr * sqrt(warmup_steps / step) (the
    Transformer schedule of Vaswani et al. 2017, normalised to peak at base_lr)."""
    step = max(int(step), 0)
    warmup_steps = int(warmup_steps)
    if step <= warmup_steps:  # (warmup_steps <= 0: no warm-up; step 0 then takes base_lr too)
        return float(base_lr) * step / warmup_steps if warmup_steps > 0 else float(base_lr)
    return float(base_lr) * math.sqrt(max(warmup_steps, 1) / step)


def step_decay(step: int, base_lr: float, every: int, factor: float) -> float:
    """base_lr * factor ** (step // every): the rate drops by `factor` at steps every, 2 every, ..."""
    if int(every) <= 0:
        raise ValueError("capgen.schedule.step_decay: every must be > 0")
    return float(base_lr) * float(factor) ** (max(int(step), 0) // int(every))


def ema_warmup(decay: float):
    """An `ema_decay` callable: t -> min(decay, (1 + t) / (10 + t)), t the number of updates the average
    has taken so far -- a young average follows the weights closely (0.1 at t = 0) and reaches `decay`
    after about 10 decay / (1 - decay) updates."""
    decay = float(decay)
    if not 0.0 < decay < 1.0:
        raise ValueError("capgen.schedule.ema_warmup: decay must be in (0, 1)")
    return lambda t: min(decay, (1.0 + t) / (10.0 + t))


class ScheduledSteps:
    """What a trainer does before each of its train steps: lr_schedule(t) -> engine.set_lr, with t the
    Adam step number of the update about to run.  The engine's counter is read once (a synchronous
    call), at the first step -- so a run resumed with Engine.set_adam_state continues its schedule --
    and counted on the host from there.  grad_clip and weight_decay (not None) are set once, at
    construction, and so is a float ema_decay; a callable ema_decay(t) -> engine.set_ema before each
    step as lr_schedule is, with t the average's update count so far (Engine.ema_info, read once).
    With every argument None nothing is ever called on the engine."""

    def __init__(self, engine, lr_schedule=None, grad_clip=None, weight_decay=None, ema_decay=None):
        self.engine, self.lr_schedule = engine, lr_schedule
        self.ema_schedule = ema_decay if callable(ema_decay) else None
        self._done = None  # Adam updates completed, once known
        self._ema_done = None  # the same for the average's updates
        if grad_clip is not None:
            engine.set_grad_clip(grad_clip)
        if weight_decay is not None:
            engine.set_weight_decay(weight_decay)
        if ema_decay is not None and self.ema_schedule is None:
            engine.set_ema(ema_decay)

    def before_step(self):
        if self.ema_schedule is not None:
            if self._ema_done is None:
                self._ema_done = int(self.engine.ema_info()[1])
            self.engine.set_ema(float(self.ema_schedule(self._ema_done)))
            self._ema_done += 1
        if self.lr_schedule is None:
            return
        if self._done is None:
            self._done = int(self.engine.adam_step_count())
        self.engine.set_lr(float(self.lr_schedule(self._done + 1)))
        self._done += 1
