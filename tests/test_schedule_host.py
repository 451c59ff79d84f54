"""capgen.schedule (pure Python) and the trainers' use of it, without a device: the schedules' shapes,
and -- on a stub engine that records every call -- that a trainer sets the learning rate exactly once
before each of its train steps, with the schedule's value at that update's Adam step number, and that
the defaults (lr_schedule=None, grad_clip=None) never call a setter."""
import math
import types

import pytest

from capgen import schedule
from capgen.models import TRANSFORMER, RolloutSelfCritic, SelfCriticNetwork


def test_warmup_inverse_sqrt_shape():
    base, W = 5e-4, 40
    lr = [schedule.warmup_inverse_sqrt(t, base, W) for t in range(0, 4 * W + 1)]
    assert lr[0] == 0.0
    for t in range(0, W + 1):  # linear up to warmup_steps
        assert lr[t] == pytest.approx(base * t / W, rel=1e-15, abs=0.0)
    assert lr[W] == base  # continuous there: both branches give base_lr
    assert schedule.warmup_inverse_sqrt(W + 1, base, W) == pytest.approx(base * math.sqrt(W / (W + 1)), rel=1e-15)
    assert abs(lr[W + 1] - lr[W]) <= base / (2 * W)  # no jump at the join (|d/dt| <= base / (2 W) after it)
    for t in range(W, 4 * W):  # non-increasing after
        assert lr[t + 1] <= lr[t]
    assert lr[4 * W] == pytest.approx(base / 2, rel=1e-15)
    assert schedule.warmup_inverse_sqrt(7, base, 0) == pytest.approx(base * math.sqrt(1 / 7), rel=1e-15)
    assert schedule.warmup_inverse_sqrt(0, base, 0) == base


def test_step_decay_boundaries():
    base, every, f = 1e-3, 10, 0.5
    want = {0: base, 1: base, 9: base, 10: base * f, 11: base * f, 19: base * f, 20: base * f * f,
            30: base * f ** 3}
    for t, v in want.items():
        assert schedule.step_decay(t, base, every, f) == pytest.approx(v, rel=1e-15), t
    with pytest.raises(ValueError):
        schedule.step_decay(1, base, 0, f)


def test_constant():
    assert [schedule.constant(t, 3e-4) for t in (0, 1, 10 ** 6)] == [3e-4] * 3


class StubEngine:
    """records (method, value) in call order; `done` Adam updates so far"""

    def __init__(self, done=0):
        self.calls, self.done = [], done

    def adam_step_count(self):
        self.calls.append(("adam_step_count", None))
        return self.done

    def set_lr(self, lr):
        self.calls.append(("set_lr", lr))

    def set_grad_clip(self, c):
        self.calls.append(("set_grad_clip", c))

    def train_step_indexed(self, *a, **k):
        self.done += 1
        self.calls.append(("step", self.done))


def _trainer(cls, eng, lr_schedule=None, grad_clip=None):
    """a trainer of class cls around the stub, built without its constructor (which creates an engine)"""
    t = cls.__new__(cls)
    t.model = types.SimpleNamespace(engine=eng)
    t.set_schedule(lr_schedule=lr_schedule, grad_clip=grad_clip)
    if cls is not TRANSFORMER:  # the SCST trainers' device work: one engine update
        t._step = lambda *a, **k: eng.train_step_indexed()
    return t


def _run(t, steps):
    store = types.SimpleNamespace(features=None, positions=None)
    for _ in range(steps):
        if isinstance(t, TRANSFORMER):
            t.train_step_resident(store, None, None)
        else:
            t.train_step(None, None, None)


@pytest.mark.parametrize("cls", [TRANSFORMER, SelfCriticNetwork, RolloutSelfCritic])
@pytest.mark.parametrize("done", [0, 37])
def test_trainer_sets_lr_once_before_each_step(cls, done):
    """done = 37: a resumed run (set_adam_state) continues the schedule at update 38"""
    sched = lambda t: schedule.warmup_inverse_sqrt(t, 5e-4, 40)  # noqa: E731
    eng = StubEngine(done)
    _run(_trainer(cls, eng, lr_schedule=sched, grad_clip=1.5), 5)
    # the clip once at construction, the engine's counter read once at the first step
    want = [("set_grad_clip", 1.5), ("adam_step_count", None)]
    for i in range(5):
        want += [("set_lr", sched(done + i + 1)), ("step", done + i + 1)]
    assert eng.calls == want


@pytest.mark.parametrize("cls", [TRANSFORMER, SelfCriticNetwork, RolloutSelfCritic])
def test_defaults_call_no_setter(cls):
    eng = StubEngine()
    _run(_trainer(cls, eng), 3)
    assert eng.calls == [("step", 1), ("step", 2), ("step", 3)]


def test_grad_clip_alone_sets_no_lr():
    eng = StubEngine()
    _run(_trainer(TRANSFORMER, eng, grad_clip=float("inf")), 2)
    assert eng.calls == [("set_grad_clip", float("inf")), ("step", 1), ("step", 2)]
