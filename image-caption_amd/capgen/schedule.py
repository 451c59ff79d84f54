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


class ScheduledSteps:
    """What a trainer does before each of its train steps: lr_schedule(t) -> engine.set_lr, with t the
    Adam step number of the update about to run.  The engine's counter is read once (a synchronous
    call), at the first step -- so a run resumed with Engine.set_adam_state continues its schedule --
    and counted on the host from there.  grad_clip (not None) is set once, at construction.  With
    lr_schedule=None and grad_clip=None nothing is ever called on the engine."""

    def __init__(self, engine, lr_schedule=None, grad_clip=None):
        self.engine, self.lr_schedule = engine, lr_schedule
        self._done = None  # Adam updates completed, once known
        if grad_clip is not None:
            engine.set_grad_clip(grad_clip)

    def before_step(self):
        if self.lr_schedule is None:
            return
        if self._done is None:
            self._done = int(self.engine.adam_step_count())
        self.engine.set_lr(float(self.lr_schedule(self._done + 1)))
        self._done += 1
